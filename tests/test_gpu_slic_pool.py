"""a3ds_label_pool_fwd / _bwd on the GPU against tests/slic_ref.py: on grid labels the forward gives
a3df_superpixel_pool_fwd's bits; on SLIC and on adversarial label maps both directions hold to float64 within 8 x the error
of the float32 restatement of the header's order (the project's rule; never below one spacing of the result), and give that
restatement's bits; the pair is adjoint within the same bounds."""
import functools

import numpy as np
import pytest
import torch

import slic_ref as S
from ann3depth_amd import models, ops

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.5)
# name: (segmentation case, h, w, C, pad channels)
CASES = {'C1': ('12x16', 5, 7, 1, 3), 'C4': ('12x16', 5, 7, 4, 4), 'C256': ('15x20', 4, 6, 256, 4),
         'model': ('240x320-10', 24, 34, 256, 0)}
KINDS = ['grid', 'slic', 'adversarial']


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@functools.lru_cache(maxsize=None)
def data(name, kind):
    seg, h, w, C, pad = CASES[name]
    n, H, W, sp = S.CASES[seg]
    total = S.geometry(H, W, sp)[2]
    rng = np.random.default_rng(sorted(CASES).index(name) * 10 + KINDS.index(kind))
    if name == 'model':
        ymap, xmap = (np.asarray(t, np.int32).copy() for t in models.fcsp_maps(H, W, h, w, 'centre'))
    else:
        ymap, xmap = (np.arange(H) * h // H).astype(np.int32), (np.arange(W) * w // W).astype(np.int32)
    labels = S.grid_labels(n, H, W, sp)
    if kind != 'grid':
        labels = S.assign64(S.image(seg), S.perturbed_centres(seg), sp, S.COMPACTNESS)[0]
    count = S.label_count(labels, sp)
    if kind == 'adversarial':
        labels = labels.copy()
        labels[0, 0, 0], labels[0, 1, 1], labels[0, 0, 2], labels[0, 3, 0] = -1, total, -2 ** 31, 2 ** 31 - 1
        labels[0, 2, 2], labels[0, H - 1, W - 1] = total - 1, 0                # far from home
        labels[n - 1][labels[n - 1] == 3] = 2                                  # a superpixel without a pixel
        count = S.label_count(labels, sp)
        assert count[n - 1, 3] == 0
        count[0, 1] = 0                                                        # one the caller declares empty, one negative
        count[0, 4] = -3
        ymap[ymap == 1] = -1                                                   # table entries out of range: no pixel maps to row 1
        ymap[H - 2], xmap[[2, W - 1]] = h, (w, -2 ** 31)
    cnt = S.pool_counts(labels, ymap, xmap, sp, h, w)
    feat = rng.standard_normal((n, h, w, C)).astype(np.float32)
    g = rng.standard_normal((n, total, C)).astype(np.float32)
    return dict(n=n, H=H, W=W, sp=sp, h=h, w=w, C=C, pad=pad, ymap=ymap, xmap=xmap, labels=labels, count=count.astype(np.int32),
                cnt=cnt, feat=feat, g=g, fwd64=S.pool_fwd64(feat, cnt, count), bwd64=S.pool_bwd64(g, cnt, count),
                fwd32=S.pool_fwd32(feat, cnt, count), bwd32=S.pool_bwd32(g, cnt, count))


def run_fwd(d, feat=None):
    """Through the kernel with `pad` NaN channels behind every cell and sentinel channels behind every pooled row."""
    feat = d['feat'] if feat is None else feat
    n, h, w, C = feat.shape
    fin = np.full((n, h, w, C + d['pad']), np.nan, np.float32)
    fin[..., :C] = feat
    out = torch.full((n, d['cnt'].shape[1], C + d['pad']), float(SENTINEL), device='cuda')
    tables = (dev(d['ymap']), dev(d['xmap']), d['sp'])
    ops.label_pool_fwd(dev(fin), tables, dev(d['labels']), dev(d['count']), out, channels=C)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert (res[..., C:] == SENTINEL).all()
    return res[..., :C]


def run_bwd(d, g=None):
    g = d['g'] if g is None else g
    n, total, C = g.shape
    gin = np.full((n, total, C + d['pad']), np.nan, np.float32)
    gin[..., :C] = g
    out = torch.full((n, d['h'], d['w'], C + d['pad']), float(SENTINEL), device='cuda')
    tables = (dev(d['ymap']), dev(d['xmap']), d['sp'])
    ops.label_pool_bwd(dev(gin), tables, dev(d['labels']), dev(d['count']), out, channels=C)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert (res[..., C:] == SENTINEL).all()
    assert (res[..., :C] != SENTINEL).all()                                    # every element is written
    return res[..., :C]


def bound(r32, r64):
    """8 x the worst error of the float32 restatement, never below one float32 spacing of the result."""
    return np.maximum(8 * np.abs(r32 - r64).max(), np.spacing(np.abs(r64).astype(np.float32)).astype(np.float64))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['C1', 'C4', 'C256'])
def test_both_directions_against_float64(name, kind):
    d = data(name, kind)
    fwd, bwd = run_fwd(d), run_bwd(d)
    bf, bb = bound(d['fwd32'], d['fwd64']), bound(d['bwd32'], d['bwd64'])
    ef, eb = np.abs(fwd - d['fwd64']), np.abs(bwd - d['bwd64'])
    print(f'label_pool {name} {kind}: forward error {ef.max():.3g} (restatement {np.abs(d["fwd32"] - d["fwd64"]).max():.3g}), '
          f'backward {eb.max():.3g} (restatement {np.abs(d["bwd32"] - d["bwd64"]).max():.3g})')
    assert (ef <= bf).all() and (eb <= bb).all()
    assert bits_equal(fwd, d['fwd32']) and bits_equal(bwd, d['bwd32'])
    lhs = (fwd.astype(np.float64) * d['g']).sum()
    rhs = (d['feat'].astype(np.float64) * bwd).sum()
    assert abs(lhs - rhs) <= (bf * np.abs(d['g'])).sum() + (bb * np.abs(d['feat'])).sum()      # the adjoint identity
    dead = d['count'] <= 0
    assert (fwd[dead].view(np.uint32) == 0).all()                              # +0, not -0, not the sentinel
    if kind == 'adversarial':
        assert dead.sum() == 3 and (d['cnt'].reshape(*dead.shape, -1).sum(-1)[dead] > 0).any()
        unmapped = d['cnt'].sum(1) == 0
        assert unmapped.any() and (bwd[unmapped].view(np.uint32) == 0).all()


@pytest.mark.parametrize('name', ['C1', 'C4', 'C256'])
def test_grid_labels_give_the_grid_poolings_bits(name):
    d = data(name, 'grid')
    assert (d['count'] == d['sp'] ** 2).all()
    x = dev(d['feat'])
    want = ops.superpixel_pool_fwd(x, (dev(d['ymap']), dev(d['xmap']), d['sp']))
    torch.cuda.synchronize()
    assert bits_equal(run_fwd(d), want.cpu().numpy())


def test_the_models_geometry_once():
    d = data('model', 'slic')
    assert d['labels'].shape == (1, 240, 320) and d['cnt'].shape[1] == ops.SLIC_MAX_SUPERPIXELS
    fwd, bwd = run_fwd(d), run_bwd(d)
    assert (np.abs(fwd - d['fwd64']) <= bound(d['fwd32'], d['fwd64'])).all() and bits_equal(fwd, d['fwd32'])
    assert (np.abs(bwd - d['bwd64']) <= bound(d['bwd32'], d['bwd64'])).all() and bits_equal(bwd, d['bwd32'])
    again = run_fwd(d), run_bwd(d)
    assert bits_equal(again[0], fwd) and bits_equal(again[1], bwd)            # the same bits on every run


def test_non_finite_values_reach_exactly_their_superpixels():
    d = data('C4', 'slic')
    clean_f, clean_b = run_fwd(d), run_bwd(d)
    feat = d['feat'].copy()
    feat[0, 2, 3, :] = np.nan
    feat[1, 0, 6, :] = np.inf
    got = run_fwd(d, feat)
    hit = np.zeros(got.shape[:2], bool)
    hit[0], hit[1] = d['cnt'][0, :, 2, 3] > 0, d['cnt'][1, :, 0, 6] > 0
    assert hit[0].any() and hit[1].any() and not hit[0].all() and not hit[1].all()
    assert np.isnan(got[0][hit[0]]).all() and (got[1][hit[1]] == np.inf).all()
    assert bits_equal(got[~hit], clean_f[~hit]) and np.isfinite(got[~hit]).all()
    g = d['g'].copy()
    g[1, 4, :] = np.nan
    gotb = run_bwd(d, g)
    cells = d['cnt'][1, 4] > 0
    assert cells.any() and not cells.all()
    assert np.isnan(gotb[1][cells]).all() and np.isfinite(gotb[1][~cells]).all() and bits_equal(gotb[0], clean_b[0])
    assert bits_equal(gotb[1][~cells], clean_b[1][~cells])


def test_wrapper_refuses_what_does_not_fit():
    d = data('C4', 'grid')
    tables = (dev(d['ymap']), dev(d['xmap']), d['sp'])
    x, labels, count = dev(d['feat']), dev(d['labels']), dev(d['count'])
    with pytest.raises(ValueError):
        ops.label_pool_fwd(x, tables, labels[:1], count)
    with pytest.raises(ValueError):
        ops.label_pool_fwd(x, tables, labels, count[:, :-1].contiguous())
    with pytest.raises(TypeError):
        ops.label_pool_fwd(x, tables, labels, count.float())
    with pytest.raises(ValueError):
        ops.label_pool_fwd(torch.zeros((2, 64, 65, 4), device='cuda'), tables, labels, count)
    assert ops.label_pool_fwd(x, tables, labels, count).shape == (2, 12, 4)
