"""Superpixel pooling's host references (tests/fcsp_ref.py) against each other and first principles, models.fcsp_maps,
ops.FcspMap's refusals and the restore checks of the two unary forms: no GPU."""
import numpy as np
import pytest
import torch

import fcsp_ref as F
from ann3depth_amd import models, ops

# (H, W, h, w, sp, align): production, both alignments; every count 1; one cell; more cells than pixels; sp 1; one superpixel
GEOMETRIES = [(240, 320, 24, 34, 40, 'centre'), (240, 320, 24, 34, 40, 'nearest'), (8, 12, 8, 12, 4, 'nearest'),
              (8, 12, 1, 1, 4, 'nearest'), (6, 6, 9, 11, 3, 'nearest'), (5, 7, 3, 4, 1, 'nearest'),
              (80, 120, 4, 9, 40, 'centre'), (16, 16, 5, 3, 16, 'nearest')]


def case(geo, n=2, C=5, seed=0):
    H, W, h, w, sp, align = geo
    ymap, xmap = models.fcsp_maps(H, W, h, w, align)
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal((n, h, w, C)).astype(np.float32)
    g = rng.standard_normal((n, (H // sp) * (W // sp), C)).astype(np.float32)
    return ymap, xmap, sp, feat, g


@pytest.mark.parametrize('geo', GEOMETRIES)
def test_float32_restatement_is_within_its_bound_of_float64(geo):
    """A sum of N float32 products, added one at a time and divided once: every term is rounded once as a product (the
    integer weight is exact), passes through at most N - 1 additions and the division, so the result is within
    (N + 1) u (1 + O(u)) of the exact one relative to sum |terms|; (N + 2) u covers the second order for N <= 2^10.
    N is the largest number of cells in a window (forward) or of superpixels on a cell (backward)."""
    ymap, xmap, sp, feat, g = case(geo)
    h, w = feat.shape[1:3]
    nf, nb = F.window_cells(ymap, xmap, sp, h, w)
    e = np.abs(F.pool_fwd32(feat, ymap, xmap, sp).astype(np.float64) - F.pool_fwd64(feat, ymap, xmap, sp))
    assert (e <= (nf + 2) * F.U * F.fwd_terms_abs(feat, ymap, xmap, sp)).all()
    e = np.abs(F.pool_bwd32(g, ymap, xmap, sp, h, w).astype(np.float64) - F.pool_bwd64(g, ymap, xmap, sp, h, w))
    assert (e <= (nb + 2) * F.U * F.pool_bwd64(np.abs(g), ymap, xmap, sp, h, w)).all()


@pytest.mark.parametrize('geo', GEOMETRIES)
def test_backward_is_the_transpose_of_the_forward(geo):
    ymap, xmap, sp, feat, g = case(geo, seed=1)
    h, w = feat.shape[1:3]
    lhs = (F.pool_fwd64(feat, ymap, xmap, sp) * g.astype(np.float64)).sum()
    rhs = (feat.astype(np.float64) * F.pool_bwd64(g, ymap, xmap, sp, h, w)).sum()
    scale = (np.abs(F.pool_fwd64(np.abs(feat), ymap, xmap, sp)) * np.abs(g)).sum()
    assert abs(lhs - rhs) <= 1e-13 * scale


@pytest.mark.parametrize('geo', GEOMETRIES)
def test_references_are_the_block_mean_of_the_upsampled_map(geo):
    """The literal definition in torch, float64: upsample by the tables, then the mean over every sp x sp block; its
    autograd gradient is the backward."""
    ymap, xmap, sp, feat, g = case(geo, seed=2)
    n, h, w, C = feat.shape
    H, W = len(ymap), len(xmap)
    f = torch.from_numpy(feat.astype(np.float64)).requires_grad_()
    up = f[:, torch.from_numpy(ymap.astype(np.int64))][:, :, torch.from_numpy(xmap.astype(np.int64))]
    pooled = up.reshape(n, H // sp, sp, W // sp, sp, C).mean(dim=(2, 4)).reshape(n, -1, C)
    np.testing.assert_allclose(pooled.detach().numpy(), F.pool_fwd64(feat, ymap, xmap, sp), rtol=1e-12, atol=1e-14)
    (pooled * torch.from_numpy(g.astype(np.float64))).sum().backward()
    np.testing.assert_allclose(f.grad.numpy(), F.pool_bwd64(g, ymap, xmap, sp, h, w), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize('geo', GEOMETRIES)
def test_counts_of_a_superpixel_sum_to_its_pixels(geo):
    H, W, h, w, sp, align = geo
    ymap, xmap = models.fcsp_maps(H, W, h, w, align)
    cy, cx = F.counts(ymap, sp, h), F.counts(xmap, sp, w)
    assert (cy.sum(1) == sp).all() and (cx.sum(1) == sp).all()
    assert (np.einsum('Ri,Qj->RQ', cy, cx) == sp * sp).all()


def test_entries_out_of_range_count_nowhere():
    cy = F.counts([-1, 0, 0, 3, 1, 2, 2, -5], 4, 3)
    assert cy.tolist() == [[2, 0, 0], [0, 1, 2]]


def test_fcsp_maps_at_the_model_size():
    assert models.fcsp_receptive() == (49, 8)                 # c0 = 24.5, jump 8: derived from DCNF_CONVS, not written down
    assert F.receptive_field(0) == (0, 49) and F.receptive_field(1) == (8, 57)
    ymap, xmap = models.fcsp_maps(240, 320, 24, 34)
    assert ymap.dtype == np.int32 and ymap.shape == (240,) and xmap.shape == (320,)
    assert np.bincount(ymap[:40]).tolist() == [29, 8, 3]
    assert (np.diff(ymap) >= 0).all() and (np.diff(xmap) >= 0).all()
    assert ymap.min() == 0 and ymap.max() == 23 and xmap.min() == 0 and xmap.max() == 33
    # the reference's own derivation: receptive fields pushed back through the layers, nearest centre by comparison
    assert F.map_size(240, 320) == (24, 34) and F.map_size(80, 120) == (4, 9)
    np.testing.assert_array_equal(ymap, F.centre_table(240, 24))
    np.testing.assert_array_equal(xmap, F.centre_table(320, 34))
    y2, x2 = models.fcsp_maps(80, 120, 4, 9)
    np.testing.assert_array_equal(y2, F.centre_table(80, 4))
    np.testing.assert_array_equal(x2, F.centre_table(120, 9))
    # at the small size of the GPU unary test the model's alignment has cells that straddle superpixel borders, on both
    # axes ('nearest' would cut the 4 x 9 cells 2 / 2 and 3 / 3 / 3, on the borders)
    assert ((F.counts(y2, 40, 4) > 0).sum(0) > 1).any() and ((F.counts(x2, 40, 9) > 0).sum(0) > 1).any()
    with pytest.raises(ValueError):
        models.fcsp_maps(240, 320, 24, 34, 'bilinear')


def test_nearest_at_equal_size_is_the_identity():
    ymap, xmap = models.fcsp_maps(12, 20, 12, 20, 'nearest')
    np.testing.assert_array_equal(ymap, np.arange(12))
    np.testing.assert_array_equal(xmap, np.arange(20))
    ymap, _ = models.fcsp_maps(240, 320, 24, 34, 'nearest')
    np.testing.assert_array_equal(ymap, np.arange(240) // 10)


def test_fcsp_map_refuses_bad_tables():
    ymap, xmap = models.fcsp_maps(8, 12, 3, 5, 'nearest')
    m = ops.FcspMap(ymap, xmap, 3, 5, 4, device='cpu')
    assert (m.H, m.W, m.h, m.w, m.sp, m.S) == (8, 12, 3, 5, 4, 6)
    assert m.ymap.dtype == torch.int32 and m.ymap.tolist() == ymap.tolist() and m.xmap.tolist() == xmap.tolist()
    dec = np.array([0, 1, 1, 0, 1, 2, 2, 2], np.int32)
    for args in ((dec, xmap, 3, 5, 4),                                       # decreasing
                 (ymap, xmap[::-1].copy(), 3, 5, 4),
                 (np.where(ymap == 2, 3, ymap), xmap, 3, 5, 4),              # out of range: h
                 (ymap, xmap - 1, 3, 5, 4),                                  # out of range: -1
                 (ymap[:7], xmap, 3, 5, 4),                                  # not a multiple of sp
                 (ymap, xmap[:0], 3, 5, 4),                                  # empty
                 (ymap, xmap, 3, 5, 0), (ymap, xmap, 3, 5, ops.FCSP_MAX_SP + 1), (ymap, xmap, 0, 5, 4),
                 (ymap.astype(np.float32), xmap, 3, 5, 4)):
        with pytest.raises(ValueError):
            ops.FcspMap(*args, device='cpu')
    with pytest.raises(ValueError):
        ops.FcspMap(ymap, xmap, 3, 5, 4, device='cpu', H=12)                 # wrong length for the image


def test_reference_unary_backward_is_the_derivative_of_its_forward():
    """fcsp_ref.unary_backward against a central difference of sum(z * dz) along a random direction, float64, at the
    small image of the GPU unary test."""
    rng = np.random.default_rng(5)
    p = F.init_params(3000, np.float64)
    for n in p:
        if n.endswith('/bias'):
            p[n] = 0.05 * rng.standard_normal(p[n].shape)
    x = rng.random((1, 80, 120, 3))
    a = F.unary_forward(p, x, 40)
    assert a['conv2d_4/pool'].shape == (1, 4, 9, 256) and a['pooled'].shape == (6, 256) and a['z'].shape == (6, 1)
    dz = rng.standard_normal((6, 1))
    g = F.unary_backward(p, a, dz, 40)
    direction = {n: rng.standard_normal(v.shape) * np.abs(v).mean() if n.endswith('/kernel') else
                 0.01 * rng.standard_normal(v.shape) for n, v in p.items()}
    want = sum((g[n] * direction[n]).sum() for n in p)
    eps = 1e-6

    def value(sign):
        q = {n: p[n] + sign * eps * direction[n] for n in p}
        return (F.unary_forward(q, x, 40)['z'] * dz).sum()
    got = (value(1) - value(-1)) / (2 * eps)
    assert abs(got - want) <= 1e-5 * abs(want), (got, want)


def test_equal_seed_draws_the_patch_forms_conv_kernels():
    from oracle import dcnf as OD
    a, b = F.init_params(7), OD.init_params(7)
    for n in a:
        if 'conv2d' in n:
            np.testing.assert_array_equal(a[n], b[n])
    assert a[OD.PREFIX + 'dense/kernel'].shape == (256, 128) and a[OD.PREFIX + 'dense_1/kernel'].shape == (128, 16)


def test_restore_across_the_two_forms_is_refused():
    """A dense/kernel of the other form: ValueError naming the flag, from params=, load_state_dict and load_tf_variables."""
    fcsp = models.DCNFReplica(1, device='cpu', unary='fcsp')
    patch = models.DCNFReplica(1, device='cpu')
    assert fcsp.unary.var('dense/kernel').shape == (256, 128) and patch.unary.var('dense/kernel').shape == (12544, 128)
    assert fcsp.unary.P == 48 and fcsp.unary.map_hw == (24, 34) and (fcsp.rows, fcsp.cols) == (6, 8)
    for rep, other in ((fcsp, patch), (patch, fcsp)):
        sd = other.state_dict()
        with pytest.raises(ValueError, match='--unary fcsp'):
            rep.load_state_dict(sd)
        with pytest.raises(ValueError, match='--unary fcsp'):
            rep.load_tf_variables(other.tf_variables())
        with pytest.raises(ValueError, match='--unary fcsp'):
            models.DCNFReplica(1, device='cpu', params=other.tf_variables(), unary=rep.unary_form)
        rep.load_state_dict(rep.state_dict())
    names = fcsp.unary.load_convs_from(patch.state_dict())
    assert len(names) == 10 and all('conv2d' in n for n in names)
    for n in names:
        assert torch.equal(fcsp.unary.group.view(fcsp.unary.group.var, n), patch.unary.group.view(patch.unary.group.var, n))
    with pytest.raises(ValueError):
        models.DCNFReplica(1, device='cpu', unary='slic')
