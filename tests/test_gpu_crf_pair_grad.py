"""a3dp_crf_loss_grad, a3dp_pair_dense_bwd and a3dp_sgd_apply_floor on the GPU (include/a3d_pairwise.h).  dr against the
float64 closed form of tests/crf_pair_grad_ref.py at the bounds that module measured (8 x the error of a float32
restatement of the kernel's own arithmetic, per grid and regime); loss, per-image loss and dz bit for bit against
a3d_crf_loss on every input; the edges of dr (bad pair index, negative determinant, overwritten pair, self pair); the
dense backward and the floored step bit for bit on exact cases.  Grids: 3x4 (fewer rows than lanes), 6x8 (the model's),
8x8 (nsp = 64 = the kernel's limit, 72 pairs: more than a wavefront).  Each test prints the worst figures it saw before it
asserts; the observed figures are kept in crf_pair_grad_ref's docstring."""
import ctypes

import numpy as np
import pytest
import torch

import crf_loss_ref as L
import crf_pair_grad_ref as G

pytestmark = pytest.mark.gpu

F = np.float32
GPU_BATCHES = [1, 5, 130]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pairs_dev(left, right):
    return dev(np.asarray(left, np.int32)), dev(np.asarray(right, np.int32))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def run(z, y, r, left, right, eps=L.EPSILON):
    """-> (mean, per, dz, dr) of crf_loss_grad, after asserting that the first three are crf_loss's bits."""
    from ann3depth_amd import ops
    args = (dev(z), dev(y), dev(r), *pairs_dev(left, right), eps)
    got = [t.cpu().numpy() for t in ops.crf_loss_grad(*args)]
    plain = [t.cpu().numpy() for t in ops.crf_loss(*args)]
    for a, b in zip(got, plain):
        np.testing.assert_array_equal(bits(a), bits(b))
    assert got[3].shape == np.shape(r) and got[3].dtype == F
    return got[0][0], got[1], got[2], got[3]


@pytest.mark.parametrize('regime', L.ACCURACY_REGIMES)
@pytest.mark.parametrize('batch', GPU_BATCHES)
@pytest.mark.parametrize('rows,cols', L.GRIDS)
def test_pair_gradient_matches_float64_and_the_loss_keeps_its_bits(rows, cols, batch, regime):
    left, right = L.pairs(rows, cols)
    z, y, r = L.draw(rows, cols, batch, regime)
    dr64 = G.reference(rows, cols, batch, regime)
    if regime == 'pivoting':
        swaps = L.restatement(rows, cols, batch, regime)[4]
        assert (swaps >= 1).all() and (batch < 5 or (swaps % 2 == 1).any())
    mean, per, dz, dr = run(z, y, r, left, right)
    err, b = G.dr_errors(dr, dr64), G.bound(rows, cols, regime)
    print(f'crf_loss_grad {rows}x{cols} batch {batch} {regime}: dr {err.max():.3g} (bound {b:.3g}), ||dr64||inf '
          f'{np.abs(dr64).max(axis=1).min():.3g} .. {np.abs(dr64).max():.3g}')
    assert np.isfinite(dr).all() and np.isfinite(per).all()
    assert err.max() <= b


def test_a_negative_determinant_is_a_nan_row_and_only_that():
    """crf_loss_ref.indefinite_batch(): dr is NaN exactly in the rows whose determinant is negative; the others are the
    bits of running them alone, a batch of 4 instead of 8: 1 / B is a power of two either way."""
    left, right = L.pairs(6, 8)
    z, y, r, det64, swaps = L.indefinite_batch()
    neg = det64 < 0
    assert neg.tolist() == [True, False] * 4 and (swaps[[1, 3]] % 2 == 1).all()
    mean, per, dz, dr = run(z, y, r, left, right)                                  # the NaN pattern of crf_loss, bit for bit
    assert np.isnan(per).tolist() == neg.tolist()
    assert np.isnan(dr).all(axis=1).tolist() == neg.tolist() and np.isnan(dr).any(axis=1).tolist() == neg.tolist()
    _, _, _, dr4 = run(z[~neg], y[~neg], r[~neg], left, right)
    np.testing.assert_array_equal(bits(dr[~neg] * F(2)), bits(dr4))
    err = G.dr_errors(dr4, G.grad64(z[~neg], y[~neg], r[~neg], left, right))
    print(f'crf_loss_grad indefinite: dr of the four positive-determinant images {err}')
    assert err.max() <= 1e-3                                      # cond_inf(A) < 1000; a lost exchange gives NaN here


@pytest.mark.parametrize('left,right', [([0, 7], [1, 1]), ([0, 0], [1, -1]), ([2, 0], [1, 1])])
def test_a_pair_index_outside_the_grid_turns_every_dr_into_nan_and_is_not_used(left, right):
    from ann3depth_amd import _lib
    lib = _lib.load()
    n, nsp = 3, 2
    z, y, r = dev(np.array([[1.0, 2.0]] * n, F)), dev(np.array([[1.1, 1.9]] * n, F)), dev(np.full((n, 2), 0.75, F))
    l, rt = pairs_dev(left, right)
    pbuf, mbuf = torch.full((n + 2,), -7.25, device='cuda'), torch.full((3,), -7.25, device='cuda')
    dbuf, rbuf = torch.full(((n + 2) * nsp,), -7.25, device='cuda'), torch.full(((n + 2) * 2,), -7.25, device='cuda')
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.a3dp_crf_loss_grad(n, nsp, z.data_ptr(), y.data_ptr(), r.data_ptr(), l.data_ptr(), rt.data_ptr(), 2, 1e-7,
                                pbuf[1:].data_ptr(), mbuf[1:].data_ptr(), dbuf[nsp:].data_ptr(), rbuf[2:].data_ptr(), stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.isnan(rbuf[2:2 + 2 * n]).all() and torch.isnan(pbuf[1:1 + n]).all() and torch.isnan(mbuf[1])
    assert torch.isnan(dbuf[nsp:nsp + n * nsp]).all()
    assert (rbuf[:2] == -7.25).all() and (rbuf[2 + 2 * n:] == -7.25).all()
    assert pbuf[0] == -7.25 and pbuf[-1] == -7.25 and (dbuf[:nsp] == -7.25).all() and (dbuf[nsp + n * nsp:] == -7.25).all()


def test_an_overwritten_pair_is_plus_zero_and_a_self_pair_is_zero():
    """crf_pair_grad_ref.edge_case(), four pairs on three nodes: (0,1) is overwritten by (1,0) and gets +0.0, the bits;
    (2,2) gets 0; the other two are held to float64 at 8 x the restatement's error on this case (EDGE_BOUND).  Then 80
    pairs on the twelve nodes of the 3x4 grid with its 'unsaturated' z, y and weights, each of its four edges many times
    in either direction (more pairs than a wavefront), at that regime's bound."""
    z, y, r, left, right = G.edge_case()
    _, per, _, dr = run(z, y, r, left, right)
    dr64 = G.grad64(z, y, r, left, right)
    print(f'crf_loss_grad overwritten / self pair: dr {dr}, float64 {dr64}')
    assert (bits(dr[:, 0]) == 0).all() and (dr[:, 2] == 0).all() and (per < 15.5).all()
    assert (np.abs(dr[:, [1, 3]]) > 1e-4).all()
    assert G.dr_errors(dr, dr64).max() <= G.EDGE_BOUND
    rng = np.random.default_rng(80)
    gl, gr = L.pairs(3, 4)
    pick = rng.integers(0, len(gl), 80)
    flip = rng.random(80) < 0.5
    left, right = np.where(flip, gr[pick], gl[pick]), np.where(flip, gl[pick], gr[pick])
    live = G.owners(left, right)
    assert 0 < live.sum() < 80 and not live[:16].all() and live[64:].any() and not live[64:].all()
    z, y, _ = L.draw(3, 4, 5, 'unsaturated')
    r = rng.uniform(2.0, 2.3, (5, 80)).astype(F)
    _, per, _, dr = run(z, y, r, left, right)
    dr64 = G.grad64(z, y, r, left, right)
    err = G.dr_errors(dr, dr64)
    print(f'crf_loss_grad 80 pairs, {live.sum()} live: dr {err.max():.3g} (bound {G.bound(3, 4, "unsaturated"):.3g})')
    assert (bits(dr[:, ~live]) == 0).all() and (dr[:, live] != 0).all()
    assert err.max() <= G.bound(3, 4, 'unsaturated')


def test_two_launches_give_the_same_bits():
    from ann3depth_amd import ops
    left, right = pairs_dev(*L.pairs(8, 8))
    z, y, r = (dev(a) for a in L.draw(8, 8, 64, 'pivoting'))
    first = [t.clone() for t in ops.crf_loss_grad(z, y, r, left, right, L.EPSILON)]
    second = ops.crf_loss_grad(z, y, r, left, right, L.EPSILON)
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------------- dense layer backward
@pytest.mark.parametrize('k', [1, 2, 3])
@pytest.mark.parametrize('n,q', [(1, 1), (1, 63), (1, 64), (5, 13), (130, 72)])
def test_pair_dense_bwd_is_exact_on_integers_and_the_same_on_every_run(n, q, k):
    """n * q = 1, 63, 64, 65 and 130 * 72 pairs (below a wavefront, one, one more, many per thread).  Every partial sum is
    an integer below 2^24: any order gives the float64 result, bit for bit.  The outputs are views into a larger buffer,
    as the replica passes them; their neighbours stay as they were.  Then a NaN in dr reaches every output."""
    from ann3depth_amd import ops
    sims, dr = G.dense_case(n * q, k)
    sims, dr = dev(sims.reshape(n, q, k)), dev(dr.reshape(n, q))
    dw64, db64 = G.dense_bwd64(sims.cpu().numpy(), dr.cpu().numpy())
    outs = []
    for _ in range(2):
        buf = torch.full((80,), -7.25, device='cuda')
        ops.pair_dense_bwd(sims, dr, buf[8:8 + k].view(k, 1), buf[72:73])
        outs.append(buf.cpu().numpy())
    np.testing.assert_array_equal(bits(outs[0]), bits(outs[1]))
    np.testing.assert_array_equal(outs[0][8:8 + k].astype(np.float64), dw64)
    assert outs[0][72] == db64
    keep = np.ones(80, bool)
    keep[8:8 + k] = keep[72] = False
    assert (outs[0][keep] == -7.25).all()
    dr.view(-1)[(n * q) // 2] = float('nan')
    dw, db = ops.pair_dense_bwd(sims, dr, torch.zeros(k, device='cuda'), torch.zeros(1, device='cuda'))
    assert torch.isnan(dw).all() and torch.isnan(db).all()


def test_pair_dense_bwd_of_real_similarities_matches_float64():
    """Not integers: 130 x 72 similarities in (0, 1) and a dr with both signs.  A sum of m float32 products in any order
    lies within (m + 1) u sum |dr| |sims| of the exact one (u = 2^-24, first order); the kernel's tree is far shorter."""
    from ann3depth_amd import ops
    rng = np.random.default_rng(13072)
    sims, dr = rng.random((130, 72, 2)).astype(F), rng.standard_normal((130, 72)).astype(F)
    dw, db = ops.pair_dense_bwd(dev(sims), dev(dr), torch.zeros((2, 1), device='cuda'), torch.zeros(1, device='cuda'))
    dw64, db64 = G.dense_bwd64(sims, dr)
    m = 130 * 72
    bound_w = (m + 1) * L.U * np.einsum('bq,bqk->k', np.abs(dr).astype(np.float64), sims.astype(np.float64))
    bound_b = (m + 1) * L.U * np.abs(dr).astype(np.float64).sum()
    e_w, e_b = np.abs(dw.cpu().numpy().reshape(-1) - dw64), abs(float(db) - db64)
    print(f'pair_dense_bwd 130x72x2: |dw - dw64| {e_w} (bound {bound_w}), |db - db64| {e_b:.3g} (bound {bound_b:.3g})')
    assert (e_w <= bound_w).all() and e_b <= bound_b


# ---------------------------------------------------------------------------------------------- floored descent step
@pytest.mark.parametrize('count', [1, 255, 256, 257, 4096 * 256 + 3])
def test_sgd_apply_floor_is_numpy_float32_bit_for_bit(count):
    """Tails around one block of 256, and more elements than the grid's 4096 blocks cover in one pass.  Element 0 lands
    exactly on the floor, a NaN variable and a NaN gradient stay NaN, about half of the rest is floored."""
    from ann3depth_amd import ops
    rng = np.random.default_rng(count)
    var, g = rng.standard_normal(count).astype(F), rng.standard_normal(count).astype(F)
    var[0], g[0] = F(0.5), F(1.0)                               # 0.5 - 0.25 * 1 = 0.25, the floor itself
    if count > 2:
        var[count // 2], g[count - 1] = np.nan, np.nan
    want = G.sgd_floor32(var, g, 0.25, 0.25)
    buf = torch.full((count + 2,), -7.25, device='cuda')
    buf[1:1 + count] = dev(var)
    ops.sgd_apply_floor(buf[1:1 + count], dev(g), 0.25, 0.25)
    got = buf.cpu().numpy()
    assert got[0] == -7.25 and got[-1] == -7.25
    np.testing.assert_array_equal(np.isnan(got[1:-1]), np.isnan(want))
    fin = ~np.isnan(want)
    np.testing.assert_array_equal(bits(got[1:-1][fin]), bits(want[fin]))
    assert got[1] == 0.25 and (count < 3 or (np.isnan(want).sum() == 2 and 0.2 < (want[fin] == 0.25).mean() < 0.8))


def test_sgd_apply_floor_without_a_floor_is_sgd_apply():
    from ann3depth_amd import ops
    rng = np.random.default_rng(3)
    var, g = rng.standard_normal(1000).astype(F), rng.standard_normal(1000).astype(F)
    a, b = dev(var), dev(var)
    ops.sgd_apply(a, dev(g), 0.1)
    ops.sgd_apply_floor(b, dev(g), 0.1, float('-inf'))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
