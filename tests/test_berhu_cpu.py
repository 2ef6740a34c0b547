"""tests/berhu_ref.py, the host references of include/a3d_berhu.h, against torch autograd (float64) of the literal loss and
against each other; the exactness conditions of the integer cases tests/test_gpu_berhu.py compares bit for bit (no GPU needed)."""
import numpy as np
import pytest
import torch

import berhu_ref as R

F = np.float32


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


@pytest.mark.parametrize('fraction', [0.2, 0.5, 1.0])
@pytest.mark.parametrize('masked', [0, 1])
def test_closed_form_gradient_is_autograd_of_the_literal_loss(masked, fraction):
    o, t = R.case(3, 257, seed=11, masked=masked)
    losses, g, c = R.loss64(o, t, masked, fraction)
    ot = torch.tensor(o.astype(np.float64), requires_grad=True)
    loss = R.literal_loss(ot, torch.tensor(t.astype(np.float64)), masked, fraction)
    loss.backward()
    assert abs(float(loss.detach()) - losses[0]) <= 1e-13 * losses[0] and losses[0] > 0
    np.testing.assert_allclose(g, ot.grad.numpy(), rtol=1e-13, atol=0)
    cnt = R.counting(t, masked)
    assert (g[~cnt] == 0).all() and (g[cnt & (o <= 0)] != 0).all() and (cnt & (o <= 0)).any()
    if fraction < 1:
        assert 0 < losses[3] < 1                       # both branches are live
    else:
        assert losses[3] == 0
    if masked:
        assert c[1] == 0 and (g[1] == 0).all()         # the sample without a finite target


@pytest.mark.parametrize('masked', [0, 1])
def test_fraction_one_is_the_l1_sum(masked):
    o, t = R.case(3, 300, seed=5, masked=masked)
    losses, g, _ = R.loss64(o, t, masked, 1.0)
    cnt = R.counting(t, masked)
    o64, t64 = o.astype(np.float64), np.where(cnt, t, 0).astype(np.float64)
    n = cnt.sum(axis=1)
    rn = np.where(n > 0, 300 / np.maximum(n, 1), 0) if masked else np.ones(3)
    l1 = (rn * np.where(cnt, np.abs(o64 - t64), 0).sum(axis=1)).sum() / 3
    assert abs(losses[0] - l1) <= 1e-14 * l1
    np.testing.assert_array_equal(g, np.where(cnt, np.sign(o64 - t64), 0) * (rn / 3)[:, None])


@pytest.mark.parametrize('b', [1, 2, 4])
def test_integer_cases_are_exact_in_float32(b):
    o, t = R.integer_case(b, 4070, seed=b)
    R.exact_conditions(o, t)
    l64, g64, c64 = R.loss64(o, t, 1, 0.5)
    l32, g32, c32 = R.loss32(o, t, 1, 0.5)
    np.testing.assert_array_equal(bits(l32), bits(l64))
    np.testing.assert_array_equal(bits(g32), bits(g64))
    assert (c32 == 2).all() and (c64 == 2).all() and l64[1] == 0.5 and l64[2] == 2
    cnt = np.isfinite(t)
    a = np.abs(o - np.where(cnt, t, 0))[cnt]
    assert set(np.unique(a)) == {0, 1, 2, 3, 4} and 0 < l64[3] < 1
    assert set(np.unique(np.abs(g64[cnt]))) == {0, 2 / b, 3 / b, 4 / b}      # s = 2 / b, e / c in {1.5, 2}


def test_float32_restatement_follows_float64_and_poison_stays_in_its_sample():
    for masked in (0, 1):
        o, t = R.case(3, 4070, seed=3, masked=masked)
        l64, g64, b_loss, b_grad = R.bound(o, t, masked, 0.2)
        print(f'berhu float32 restatement (3,4070) masked={masked}: loss bound {b_loss:.2e}, gradient bound {b_grad:.2e}')
        assert 0 < b_loss < 1e-5 and 0 < b_grad < 1e-5
    o, t = R.case(3, 64, seed=4, masked=0)
    clean = R.loss32(o, t, 0, 0.2)
    for bad_o, bad_t in ((np.nan, None), (np.inf, None), (None, np.nan)):
        o2, t2 = o.copy(), t.copy()
        if bad_o is not None:
            o2[1, 7] = bad_o
        else:
            t2[1, 7] = bad_t
        for fn in (R.loss32, R.loss64):
            losses, g, c = fn(o2, t2, 0, 0.2)
            assert np.isnan(g[1]).all() and np.isnan(c[1]) and np.isnan([losses[0], losses[2], losses[3]]).all()
            assert losses[1] == 1
        np.testing.assert_array_equal(bits(R.loss32(o2, t2, 0, 0.2)[1][[0, 2]]), bits(clean[1][[0, 2]]))
