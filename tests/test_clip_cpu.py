"""tests/clip_ref.py, the host restatement of include/a3d_clip.h, against torch.nn.utils.clip_grad_norm_ on float64 tensors, and
its skip rule.  No GPU."""
import numpy as np
import pytest
import torch

import clip_ref as CR


def torch_clipped(g, C):
    """The gradients torch leaves after clip_grad_norm_(max_norm=C), in float64, split over two parameters."""
    cut = g.size // 3
    params = [torch.nn.Parameter(torch.zeros(n, dtype=torch.float64)) for n in (cut, g.size - cut)]
    params[0].grad = torch.from_numpy(g[:cut].astype(np.float64))
    params[1].grad = torch.from_numpy(g[cut:].astype(np.float64))
    total = torch.nn.utils.clip_grad_norm_(params, C)
    return np.concatenate([p.grad.numpy() for p in params]), float(total)


@pytest.mark.parametrize('count', [1, 5, 1027])
def test_clipped_gradients_agree_with_torch(count):
    """torch multiplies by C / (n + 1e-6), the definition by fl32(C / n).  With n >= 1 the first factor is C / n times
    1 / (1 + 1e-6 / n), at most 1e-6 relative below it; the rounding to float32 moves the second by at most 2^-24 relative; the
    float64 roundings of either side (the norm's sum, the division) are below 2^-45.  So every clipped element agrees to a
    relative 1e-6 + 2^-23."""
    rng = np.random.default_rng(count)
    g = (rng.standard_normal(count) * 3).astype(np.float32)
    g[0] = 2.0                                                  # the norm is >= 1 whatever the draw
    n = float(np.sqrt(CR.sumsq(g)))
    assert n >= 1
    for C in (n / 2, n / 7.3, 1e-3):
        c = CR.clip(g, 1.0, C)
        assert c.skip == 0 and c.scale < 1
        want, total = torch_clipped(g, float(np.float32(C)))
        assert abs(total - n) <= 1e-12 * n and abs(float(c.norm) - n) <= 2.0 ** -23 * n
        got = g.astype(np.float64) * np.float64(c.scale)
        assert (np.abs(got - want) <= (1e-6 + 2.0 ** -23) * np.abs(want)).all()
        assert np.linalg.norm(got) <= float(np.float32(C)) * (1 + 2.0 ** -23)


@pytest.mark.parametrize('count', [1, 5, 1027])
def test_below_the_threshold_nothing_changes(count):
    rng = np.random.default_rng(100 + count)
    g = (rng.standard_normal(count) * 3).astype(np.float32)
    g[0] = 2.0
    n = float(np.sqrt(CR.sumsq(g)))
    for C in (2 * n, 1e30, np.inf):
        for gs in (1.0, 0.5):
            c = CR.clip(g, gs, C / gs)
            assert c.skip == 0 and c.scale.view(np.uint32) == np.float32(gs).view(np.uint32)
        want, _ = torch_clipped(g, C)
        assert (want == g.astype(np.float64)).all()             # torch's clamped coefficient is exactly 1


def test_equality_does_not_clip_and_one_ulp_below_does():
    g = np.array([3, 4, 0, 0, 0], np.float32)
    assert CR.clip(g, 1.0, 5.0) == CR.Clip(25.0, np.float32(5), np.float32(1), 0)
    assert CR.clip(g, 1.0, 2.5).scale == np.float32(0.5)
    assert CR.clip(g, 1.0, np.nextafter(np.float32(5), np.float32(0))).scale < 1
    assert CR.clip(g, 0.5, 2.5).scale == np.float32(0.5) and CR.clip(g, 0.5, 1.25).scale == np.float32(0.25)
    assert CR.clip(np.zeros(3, np.float32), 1.0, 1.0) == CR.Clip(0.0, np.float32(0), np.float32(1), 0)


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize('where', [0, 3, 6])
def test_a_non_finite_element_anywhere_skips(bad, where):
    g = np.arange(1, 8, dtype=np.float32)
    g[where] = bad
    for C in (1.0, np.inf):
        c = CR.clip(g, 0.5, C)
        assert c.skip == 1 and c.scale == 0 and not np.isfinite(c.sumsq)
    var = np.ones(7, np.float32)
    c = CR.clip(g, 1.0, 1.0)
    assert (CR.sgd(var, g, 0.1, c) == var).all() and (CR.momentum(var, var, g, 0.1, 0.9, c)[1] == var).all()


def test_a_norm_beyond_float32_is_reported_as_inf_and_is_no_skip():
    g = np.full(4, np.finfo(np.float32).max, np.float32)
    c = CR.clip(g, 1.0, 1.0)
    assert c.skip == 0 and np.isinf(c.norm) and np.isfinite(c.sumsq) and 0 < c.scale < 1e-38


def test_the_rules_take_the_scale():
    rng = np.random.default_rng(5)
    var, acc, g = (rng.standard_normal(9).astype(np.float32) for _ in range(3))
    c = CR.clip(g, 1.0, 0.5)
    import momentum_ref as MR
    for got, want in zip(CR.momentum(var, acc, g, 0.1, 0.9, c), MR.step(var, acc, g, 0.1, 0.9, c.scale)):
        assert (got == want).all()
    lr = np.float32(0.1) * c.scale
    assert (CR.sgd(var, g, 0.1, c) == var - lr * g).all()
    assert (CR.sgd(var, g, 0.1, c, floor=0.0) == np.maximum(var - lr * g, np.float32(0))).all()
