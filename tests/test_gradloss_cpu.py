"""tests/gradloss_ref.py, the host reference of include/a3d_gradloss.h, against torch autograd (float64) of the literal loss
written with torch.where, masked and unmasked; at weight 0 against tests/valid_ref.py; and the error of its float32 run on the
cases tests/test_gpu_gradloss.py uses, which sets the kernels' tolerance there (printed here; no GPU needed)."""
import numpy as np
import pytest
import torch

import gradloss_ref as G
import valid_ref as V

SHAPES = [(2, 1, 1), (2, 1, 7), (2, 7, 1), (3, 3, 5), (2, 2, 600), (65, 3, 11), (3, 55, 74)]     # test_gpu_gradloss.py's


def literal_loss(o, t, h, w, masked, weight):
    """The loss as one would write it in torch: (total, silog part, gradient part)."""
    b = o.shape[0]
    o, t = o.reshape(b, h, w), t.reshape(b, h, w)
    zero = torch.zeros((), dtype=o.dtype)
    valid = torch.isfinite(t) if masked else torch.ones_like(t, dtype=torch.bool)
    lo = torch.log(o + G.EPS)
    lo = torch.where(torch.isnan(lo), zero, lo)
    lt = torch.log(torch.where(valid, t, torch.ones_like(t)) + G.EPS)
    lt = torch.where(torch.isnan(lt), zero, lt)
    d = torch.where(valid, lo - lt, zero)
    s2, s1 = (d * d).sum(dim=(1, 2)), d.sum(dim=(1, 2))
    vh, vv = valid[:, :, 1:] & valid[:, :, :-1], valid[:, 1:] & valid[:, :-1]
    sg = (torch.where(vh, (d[:, :, 1:] - d[:, :, :-1]) ** 2, zero).sum(dim=(1, 2))
          + torch.where(vv, (d[:, 1:] - d[:, :-1]) ** 2, zero).sum(dim=(1, 2)))
    if masked:
        n = valid.sum(dim=(1, 2)).to(o.dtype)
        m = (vh.sum(dim=(1, 2)) + vv.sum(dim=(1, 2))).to(o.dtype)
        pairs = h * (w - 1) + (h - 1) * w
        silog = torch.where(n > 0, (h * w / n.clamp(min=1)) * (s2 - (0.5 / n.clamp(min=1)) * s1 ** 2), zero)
        grad = torch.where(m > 0, (pairs / m.clamp(min=1)) * sg, zero)
    else:
        silog, grad = s2 - G.SILOG_C * s1 ** 2, sg
    return silog.mean() + weight * grad.mean(), silog.mean(), grad.mean()


@pytest.mark.parametrize('masked', [0, 1])
@pytest.mark.parametrize('b,h,w', SHAPES)
def test_reference_is_autograd_of_the_literal_loss(b, h, w, masked):
    o, t = (a.astype(np.float64) for a in G.loss_case(b, h, w, seed=b + h))
    if not masked:
        t = np.nan_to_num(t, nan=0.37, posinf=0.61)
    for weight in (0.0, 0.5, 1.0):
        ot = torch.from_numpy(o.copy()).requires_grad_(True)
        total, silog, grad = literal_loss(ot, torch.from_numpy(t), h, w, masked, weight)
        total.backward()
        ref = G.grad_loss_fwd(o, t, h, w, masked, weight)
        for got, want in ((total, ref[0]), (silog, ref[2]), (grad, ref[3])):
            assert abs(float(got.detach()) - want) <= 1e-12 * max(abs(want), 1e-30)
        assert ref[1] == (np.isfinite(t).mean() if masked else 1.0)
        g = G.grad_loss_bwd(o, t, h, w, masked, weight)
        assert G.rel_l2(g, ot.grad.numpy().reshape(b, -1)) < 1e-12
        hole = ~np.isfinite(t)
        assert (g[o < -1e-8] == 0).all() and (not masked or ((g[hole] == 0).all() and (g[-1] == 0).all()))
        assert h * w == 1 or (g[0] != 0).any()
    if h * w == 1:
        assert ref[3] == 0                                                   # no pair


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_weight_zero_is_the_masked_loss_of_valid_ref(dtype):
    o, t = (a.astype(dtype) for a in G.loss_case(3, 55, 74, seed=7))
    total, frac, silog, _ = G.grad_loss_fwd(o, t, 55, 74, 1, 0.0)
    want, want_frac = V.masked_silog_fwd(o, t)
    assert total == silog == want and frac == want_frac
    np.testing.assert_array_equal(G.grad_loss_bwd(o, t, 55, 74, 1, 0.0), V.masked_silog_bwd(o, t))


def test_the_cases_are_what_the_gpu_tests_need():
    for b, h, w in SHAPES:
        o, t = G.loss_case(b, h, w, seed=b + h)
        valid = np.isfinite(t)
        assert o.dtype == t.dtype == np.float32 and not valid[-1].any() and valid[:-1, 0].all()
        assert (np.abs(o) > 0.05).all() and (np.abs(o) < 1).all() and (o + np.float32(1e-8) != 0).all()
        assert (t[valid] > 0.05).all() and (t[valid] < 1).all()
        if h * w > 1:
            assert (o < -1e-8).any() and not valid.reshape(b, h, w)[:, -1, -1].any() and (np.isinf(t).any() or b * h * w < 1000)
        o0, t0 = G.loss_case(b, h, w, seed=b + h, invalid=0)
        assert np.isfinite(t0).all()
    o, t = G.constant_case(3, 5, 7, 1)
    assert G.grad_loss_fwd(o, t, 5, 7, 1, 1.0)[3] == 0 and not np.isfinite(t).all()


def test_print_the_float32_restatements_error():
    """8 x these figures are the bounds of tests/test_gpu_gradloss.py; none may be looser than the 2e-6 / 1e-5 of
    tests/test_gpu_masked_loss.py."""
    for b, h, w in SHAPES:
        for masked in (0, 1):
            o, t = G.loss_case(b, h, w, seed=b + h, invalid=None if masked else 0)
            _, b_loss, b_grad = G.tolerances(o, t, h, w, masked)
            print(f'gradloss float32 restatement ({b},{h},{w}) masked={masked}: loss {b_loss / 8:.2e} gradient rel-L2 '
                  f'{b_grad / 8:.2e}')
            assert 0 < b_loss <= 2e-6 and 0 < b_grad <= 1e-5
