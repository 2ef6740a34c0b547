"""The SLIC segmentation and the label statistics on the GPU (include/a3d_slic.h) against tests/slic_ref.py.

Counts, histograms and labels are integers and must be exact; coordinate means are the float64 mean after one rounding;
colour means of inputs in [0, 1] lie within (count + 1) 2^-24 relative of the float64 mean, the bound of any summation
order plus the division.  An assignment is held to the float64 reference on DECIDED pixels (the two best distances differ
by more than 64 * 2^-24 of the larger: a D is about 8 float32 operations on non-negative terms, 16 * 2^-24 covers two of
them, 64 leaves 4x) and to one of the two best on the others, of which tests/test_slic_cpu.py shows there are at most 1 %.
On the small cases the kernels also give the bits of the float32 restatements, whose order the header fixes."""
import functools

import numpy as np
import pytest
import torch

import slic_ref as S
from ann3depth_amd import ops

pytestmark = pytest.mark.gpu

SMALL = ['12x16', '8x8', '15x20']
LARGE = ['240x320-10', '240x320-40']
SENTINEL = np.float32(-12345.5)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@functools.lru_cache(maxsize=None)
def data(name):
    """Image, perturbed centres, a label map with every kind of label the contract excludes, and its references; computed
    once and shared (never written to)."""
    n, H, W, sp = S.CASES[name]
    rows, cols, total = S.geometry(H, W, sp)
    x, ce = S.image(name), S.perturbed_centres(name)
    a64, second, decided = S.assign64(x, ce, sp, S.COMPACTNESS)
    labels = a64.copy()
    labels[0, 0, 0], labels[0, 1, 1] = -1, total                               # negative, >= S
    labels[0, 0, 2], labels[0, 3, 0] = -2 ** 31, 2 ** 31 - 1
    if rows > 2:
        labels[0, 2, 2], labels[0, H - 1, W - 1] = total - 1, 0                # far from home
    empty = total - 2
    labels[n - 1][labels[n - 1] == empty] = empty + 1                          # a superpixel without a pixel, anchor included
    cnt, mean64 = S.label_mean64(x, labels, sp)
    ce64, _ = S.update64(x, labels, sp)
    assert cnt[n - 1, empty] == 0 and (np.delete(cnt[n - 1], empty) > 0).all() and cnt[0].sum() < H * W
    return dict(x=x, ce=ce, a64=a64, second=second, decided=decided, labels=labels, cnt=cnt, mean64=mean64, ce64=ce64,
                hist=S.label_hist(x, labels, sp), empty=empty)


def check_statistics(name, restated):
    n, H, W, sp = S.CASES[name]
    d = data(name)
    x, labels, cnt, empty = dev(d['x']), dev(d['labels']), d['cnt'], d['empty']
    live = cnt > 0
    mean, count = ops.label_mean(x, sp, labels)
    mean, count = host(mean), host(count)
    assert count.dtype == np.int32 and (count == cnt).all()
    err = np.abs(mean[live] - d['mean64'][live]) / np.abs(d['mean64'][live])
    print(f'label_mean {name}: worst error {err.max() / S.U:.2f} u, worst bound use {(err / (cnt[live][:, None] + 1)).max() / S.U:.3f}')
    assert (err <= (cnt[live][:, None] + 1) * S.U).all()
    assert np.isnan(mean[~live]).all() and (~live).sum() == 1
    hist = host(ops.label_hist(x, sp, labels))
    assert hist.dtype == np.float32 and (hist == d['hist']).all() and (hist.sum(-1) == cnt).all()
    centres = torch.full((n, cnt.shape[1], 5), float(SENTINEL), device='cuda')
    got, count2 = ops.slic_update(x, sp, labels, centres)
    assert got is centres
    got = host(got)
    assert (host(count2) == cnt).all()
    assert (got[~live] == SENTINEL).all()                                     # a row without pixels is left alone
    assert (got[live][:, :2] == d['ce64'][live][:, :2].astype(np.float32)).all()      # one rounding of the exact mean
    assert bits_equal(got[live][:, 2:], mean[live])                           # the same reduction body
    for c in (1, 4):                                                           # the target (c = 1) and the widest pixel
        v = np.concatenate([d['x'], d['x'][..., :1] * 3 + 1], -1)[..., -c:].copy()
        m, k = ops.label_mean(dev(v), sp, labels)
        m64 = S.label_mean64(v, d['labels'], sp)[1]
        assert (host(k) == cnt).all() and np.isnan(host(m)[~live]).all()
        assert (np.abs(host(m)[live] - m64[live]) <= (cnt[live][:, None] + 1) * S.U * np.abs(m64[live])).all()
        if restated:
            assert bits_equal(host(m), S.label_mean32(v, d['labels'], sp)[1])
    if restated:
        assert bits_equal(mean, S.label_mean32(d['x'], d['labels'], sp)[1])
        assert bits_equal(got[live], S.update32(d['x'], d['labels'], sp)[0][live])


def check_assign(name, restated):
    n, H, W, sp = S.CASES[name]
    d = data(name)
    got = host(ops.slic_assign(dev(d['x']), sp, dev(d['ce']), S.COMPACTNESS))
    dec = d['decided']
    print(f'slic_assign {name}: {(~dec).sum()} of {dec.size} pixels undecided, '
          f'{(got != d["a64"]).sum()} labels differ from float64')
    assert (~dec).sum() <= 0.01 * dec.size
    assert got.dtype == np.int32 and (got[dec] == d['a64'][dec]).all()
    assert ((got == d['a64']) | (got == d['second'])).all()
    assert S.counts_mask(got, sp).all()
    if restated:
        assert (got == S.assign32(d['x'], d['ce'], sp, S.COMPACTNESS)).all()


@pytest.mark.parametrize('name', SMALL)
def test_statistics_of_a_label_map(name):
    check_statistics(name, True)


@pytest.mark.parametrize('name', SMALL)
def test_assignment_against_float64(name):
    check_assign(name, True)


@pytest.mark.parametrize('name', LARGE)
def test_the_models_image_once(name):
    n, H, W, sp = S.CASES[name]
    check_statistics(name, False)
    check_assign(name, False)
    x = dev(data(name)['x'])
    labels, centres, count = ops.slic_segment(x, sp, 2, S.COMPACTNESS)
    lab = host(labels)
    grid = S.grid_labels(n, H, W, sp)
    assert S.counts_mask(lab, sp).all() and (lab[:, S.anchors(H, W, sp)] == grid[:, S.anchors(H, W, sp)]).all()
    assert (host(count) == S.label_count(lab, sp)).all() and (host(count) > 0).all() and host(count).sum() == H * W
    assert (lab != grid).any() and np.isfinite(host(centres)).all()


def test_ties_nan_centres_anchor_and_constant_image():
    name = '12x16'
    n, H, W, sp = S.CASES[name]
    d = data(name)
    x = dev(d['x'])
    total = S.geometry(H, W, sp)[2]
    grid, anc = S.grid_labels(n, H, W, sp), np.broadcast_to(S.anchors(H, W, sp), (n, H, W))
    same = np.tile(np.array([5.5, 7.5, 0.5, 0.5, 0.5], np.float32), (n, total, 1))
    lowest = np.array([[S.candidates(y, xx, H, W, sp)[0] for xx in range(W)] for y in range(H)])
    got = host(ops.slic_assign(x, sp, dev(same), S.COMPACTNESS))
    assert (got == np.where(anc, grid, lowest[None])).all()                   # exact ties go to the lowest index
    assert (host(ops.slic_assign(x, sp, dev(np.full_like(same, np.nan)), S.COMPACTNESS)) == grid).all()
    ce = d['ce'].copy()
    ce[:, 5, 3] = np.nan                                                       # one NaN in a centre: that candidate is skipped
    ce[:, 6] = np.inf
    got = host(ops.slic_assign(x, sp, dev(ce), S.COMPACTNESS))
    assert (got == S.assign32(d['x'], ce, sp, S.COMPACTNESS)).all()
    assert not np.isin(got[~anc], (5, 6)).any() and (got[anc] == grid[anc]).all()
    far = d['ce'].copy()
    far[..., :2] += 1000                                                       # every centre far away: the anchors still hold
    assert (host(ops.slic_assign(x, sp, dev(far), S.COMPACTNESS))[anc] == grid[anc]).all()
    flat = torch.full((n, H, W, 3), 0.3, device='cuda')
    for iters in (0, 1, 5):
        labels, centres, count = ops.slic_segment(flat, sp, iters, S.COMPACTNESS)
        assert (host(labels) == grid).all() and (host(count) == sp * sp).all()


@pytest.mark.parametrize('name', SMALL)
def test_segment_is_the_call_sequence_and_repeats(name):
    n, H, W, sp = S.CASES[name]
    x = dev(data(name)['x'])
    iters = 4
    labels, centres, count = ops.slic_segment(x, sp, iters, S.COMPACTNESS)
    again = ops.slic_segment(x, sp, iters, S.COMPACTNESS)
    assert (host(labels) == host(again[0])).all() and bits_equal(host(centres), host(again[1]))
    assert (host(count) == host(again[2])).all()
    grid = S.grid_labels(n, H, W, sp)
    l0, c0, k0 = ops.slic_segment(x, sp, 0, S.COMPACTNESS)
    assert (host(l0) == grid).all() and (host(k0) == sp * sp).all()
    assert bits_equal(host(c0), S.update32(data(name)['x'], grid, sp)[0])     # the grid and its block means
    # by hand, and in lockstep: each assignment against the reference fed the kernel's own centres
    lab = dev(grid)
    ce, cnt = ops.slic_update(x, sp, lab, torch.full((n, int(grid.max()) + 1, 5), float(SENTINEL), device='cuda'))
    moved = 0
    for _ in range(iters):
        ce_host = host(ce).copy()
        lab = ops.slic_assign(x, sp, ce, S.COMPACTNESS, lab)
        a64, second, dec = S.assign64(data(name)['x'], ce_host, sp, S.COMPACTNESS)
        got = host(lab)
        assert (~dec).sum() <= 0.01 * dec.size
        assert (got[dec] == a64[dec]).all() and ((got == a64) | (got == second)).all()
        moved += (got != grid).sum()
        ce, cnt = ops.slic_update(x, sp, lab, ce, cnt)
        assert bits_equal(host(ce), S.update32(data(name)['x'], got, sp, ce_host)[0])
    assert moved > 0
    assert (host(lab) == host(labels)).all() and bits_equal(host(ce), host(centres)) and (host(cnt) == host(count)).all()


def test_wrappers_refuse_what_does_not_fit():
    x = torch.zeros((2, 12, 16, 3), device='cuda')
    labels = torch.zeros((2, 12, 16), dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError):
        ops.label_mean(x, 5, labels)
    with pytest.raises(ValueError):
        ops.label_mean(x, 4, labels[:1])
    with pytest.raises(TypeError):
        ops.label_mean(x, 4, labels.long())
    with pytest.raises(ValueError):
        ops.label_hist(x[..., :2].contiguous(), 4, labels)
    with pytest.raises(ValueError):
        ops.slic_segment(x, 4, -1)
    with pytest.raises(ValueError):
        ops.slic_segment(x, 4, 2, compactness=float('nan'))
    with pytest.raises(ValueError):
        ops.slic_assign(x, 4, torch.zeros((2, 12, 4), device='cuda'), 0.1)
    with pytest.raises(ValueError):
        ops.slic_update(torch.zeros((1, 64, 512, 3), device='cuda'), 64, torch.zeros((1, 64, 512), dtype=torch.int32, device='cuda'), None)
    vals = torch.arange(24, dtype=torch.float32, device='cuda').reshape(2, 12)
    lab = dev(S.grid_labels(2, 12, 16, 4))
    assert (host(ops.paint_labels(vals, lab)) == host(vals)[np.arange(2)[:, None, None], S.grid_labels(2, 12, 16, 4)]).all()
