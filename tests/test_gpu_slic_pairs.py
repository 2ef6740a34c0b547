"""a3ds_pair_similarity on the GPU against tests/slic_ref.py: within 8 x the error of the float32 restatement of the
header's order of float64 (the project's rule; never below one float32 spacing of the result), NaN for a pair with a bad
index and only for it, and count used as the header states (a frequency is hist / count, whatever hist sums to)."""
import functools

import numpy as np
import pytest
import torch

import slic_ref as S
from ann3depth_amd import models, ops

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def data(name):
    n, H, W, sp = S.CASES[name]
    rows, cols, total = S.geometry(H, W, sp)
    x = S.image(name)
    labels = S.assign64(x, S.perturbed_centres(name), sp, S.COMPACTNESS)[0]
    count, mean3 = S.label_mean32(x, labels, sp) if total < 100 else (lambda c, m: (c.astype(np.int32), m.astype(np.float32)))(
        *S.label_mean64(x, labels, sp))
    hist = S.label_hist(x, labels, sp).astype(np.float32)
    if total > 100:
        left, right = (np.array(v, np.int32) for v in models.dcnf_pair_indices(rows, cols))
    else:                                      # every horizontal and vertical neighbour pair, and one self pair
        cells = np.arange(total).reshape(rows, cols)
        left = np.concatenate([cells[:, :-1].ravel(), cells[:-1].ravel(), [total - 1]]).astype(np.int32)
        right = np.concatenate([cells[:, 1:].ravel(), cells[1:].ravel(), [total - 1]]).astype(np.int32)
    return dict(mean3=mean3, hist=hist, count=count, left=left, right=right, dw=np.array([0.7, 0.4], np.float32),
                db=np.array([0.05], np.float32), total=total)


def run(d, gamma=1.0, **over):
    a = {**d, **over}
    sims, r = ops.label_pair_similarity(dev(a['mean3']), dev(a['hist']), dev(a['count']), dev(a['left']), dev(a['right']),
                                        dev(a['dw']), dev(a['db']), gamma)
    torch.cuda.synchronize()
    return sims.cpu().numpy(), r.cpu().numpy()


def check(got, r32, r64):
    tol = np.maximum(8 * np.abs(r32 - r64).max(), np.spacing(np.abs(r64).astype(np.float32)).astype(np.float64))
    print(f'label_pair_similarity: worst error {np.abs(got - r64).max():.3g}, restatement {np.abs(r32 - r64).max():.3g}')
    assert (np.abs(got - r64) <= tol).all()


@pytest.mark.parametrize('name', ['12x16', '8x8', '15x20', '240x320-10'])
@pytest.mark.parametrize('gamma', [1.0, 2.5])
def test_similarities_against_float64(name, gamma):
    d = data(name)
    args = (d['mean3'], d['hist'], d['count'], d['left'], d['right'], d['dw'], d['db'], gamma)
    (s64, r64), (s32, r32) = S.pair_similarity64(*args), S.pair_similarity32(*args)
    sims, r = run(d, gamma)
    assert sims.shape == s64.shape and r.shape == r64.shape and sims.dtype == r.dtype == np.float32
    check(sims, s32, s64)
    check(r, r32, r64)
    assert (sims > 0).all() and (sims <= 1).all()
    again = run(d, gamma)
    assert (again[0].view(np.uint32) == sims.view(np.uint32)).all() and (again[1].view(np.uint32) == r.view(np.uint32)).all()


def test_bad_indices_give_nan_for_their_pair_only():
    d = data('12x16')
    clean_s, clean_r = run(d)
    left, right = d['left'].copy(), d['right'].copy()
    left[1], right[2], left[5], right[6] = -1, d['total'], -2 ** 31, 2 ** 31 - 1
    sims, r = run(d, left=left, right=right)
    bad = np.zeros(left.size, bool)
    bad[[1, 2, 5, 6]] = True
    assert np.isnan(sims[:, bad]).all() and np.isnan(r[:, bad]).all()
    assert (sims[:, ~bad].view(np.uint32) == clean_s[:, ~bad].view(np.uint32)).all()
    assert (r[:, ~bad].view(np.uint32) == clean_r[:, ~bad].view(np.uint32)).all()


def test_count_is_the_divisor_and_zero_gives_nan():
    d = data('12x16')
    count = d['count'].copy()
    count[0] *= 2                                                              # not what hist sums to: still the divisor
    count[1, d['left'][0]] = 0
    args = (d['mean3'], d['hist'], count, d['left'], d['right'], d['dw'], d['db'], 1.0)
    (s64, r64), (s32, r32) = S.pair_similarity64(*args), S.pair_similarity32(*args)
    sims, r = run(d, count=count)
    dead = np.zeros(r.shape, bool)
    dead[1] = (d['left'] == d['left'][0]) | (d['right'] == d['left'][0])
    assert dead.any() and np.isnan(sims[..., 1][dead]).all() and np.isnan(r[dead]).all() and np.isnan(s64[..., 1][dead]).all()
    assert np.isfinite(sims[..., 0]).all() and np.isfinite(r[~dead]).all()
    check(sims[~dead], s32[~dead], s64[~dead])
    check(r[~dead], r32[~dead], r64[~dead])
    assert (sims[0, :-1, 1] > run(d)[0][0, :-1, 1]).all()                      # half the frequencies: nearer histograms
    assert sims[0, -1, 1] == 1                                                 # the self pair


def test_wrapper_refuses_what_does_not_fit():
    d = data('12x16')
    t = {k: dev(d[k]) for k in ('mean3', 'hist', 'count', 'left', 'right', 'dw', 'db')}
    with pytest.raises(ValueError):
        ops.label_pair_similarity(t['mean3'], t['hist'][:, :-1].contiguous(), t['count'], t['left'], t['right'], t['dw'], t['db'])
    with pytest.raises(ValueError):
        ops.label_pair_similarity(t['mean3'], t['hist'], t['count'], t['left'], t['right'][:-1], t['dw'], t['db'])
    with pytest.raises(TypeError):
        ops.label_pair_similarity(t['mean3'], t['hist'], t['count'].float(), t['left'], t['right'], t['dw'], t['db'])
    with pytest.raises(ValueError):
        ops.label_pair_similarity(t['mean3'], t['hist'], t['count'], t['left'], t['right'], torch.zeros(3, device='cuda'), t['db'])
