"""a3df_superpixel_pool_fwd / _bwd on the GPU against tests/fcsp_ref.py: bit for bit against the float32 restatement of
the header's operation order on random normal data, and the exact integer result on small-integer data (|v| <= 4096: every
sum of weight * value stays within 2^24 and is exact in any order, so only the one division rounds)."""
import functools

import numpy as np
import pytest
import torch

import fcsp_ref as F
from ann3depth_amd import models, ops

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.5)
CAP = ops.FCSP_MAX_SP
# name: (H, W, h, w, sp, align, n, C, pad channels, float offset of the base pointers)
CASES = {
    'model-centre': (240, 320, 24, 34, 40, 'centre', 2, 256, 0, 0),      # the model's geometry; 16-byte path
    'model-nearest': (240, 320, 24, 34, 40, 'nearest', 2, 256, 0, 0),
    'C1-pad3': (24, 36, 5, 7, 12, 'nearest', 2, 1, 3, 0),                # scalar path, tails, misaligned rows
    'C3-pad3': (24, 36, 5, 7, 12, 'nearest', 2, 3, 3, 0),
    'C65-pad3': (24, 36, 5, 7, 12, 'nearest', 2, 65, 3, 0),
    'C8-pad4': (24, 36, 5, 7, 12, 'nearest', 2, 8, 4, 0),                # 16-byte path with pad channels
    'C8-offset': (24, 36, 5, 7, 12, 'nearest', 2, 8, 0, 1),              # aligned strides, base pointer off the 16-byte grid
    'C259': (8, 12, 3, 2, 4, 'nearest', 1, 259, 0, 0),                   # scalar path, a second channel pass (> 256 lanes)
    'C1100': (8, 12, 3, 2, 4, 'nearest', 1, 1100, 0, 0),                 # 16-byte path, a second channel pass (275 lanes)
    'every-count-1': (8, 12, 8, 12, 4, 'nearest', 2, 5, 0, 0),
    'one-cell': (8, 12, 1, 1, 4, 'nearest', 2, 5, 0, 0),
    'cells-without-pixels': (6, 6, 9, 11, 3, 'nearest', 2, 4, 0, 0),
    'sp1': (5, 7, 3, 4, 1, 'nearest', 2, 4, 0, 0),
    'one-superpixel': (16, 16, 5, 3, 16, 'nearest', 2, 6, 0, 0),
    'sp-cap': (CAP, 2 * CAP, 7, 13, CAP, 'nearest', 1, 8, 0, 0),
    'many-superpixels': (70, 3, 4, 2, 1, 'nearest', 1, 4, 0, 0),        # more than 64 superpixel rows: the backward's chunks
}


def bits_equal(a, b):
    """The same float32 bits, any NaN standing for any NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def run_fwd(feat, ymap, xmap, sp, pad=0, offset=0, tables=None):
    """feat [n,h,w,C] host -> pooled [n,S,C] host through the kernel, with `pad` NaN channels behind every pixel of the
    input and sentinel channels behind every row of the output, which must come back untouched."""
    n, h, w, C = feat.shape
    S = (len(ymap) // sp) * (len(xmap) // sp)
    fin = np.full((n, h, w, C + pad), np.nan, np.float32)
    fin[..., :C] = feat
    store = torch.empty(fin.size + offset, device='cuda')
    x = store[offset:].view(n, h, w, C + pad)
    x.copy_(torch.from_numpy(fin))
    ostore = torch.full((n * S * (C + pad) + offset,), float(SENTINEL), device='cuda')
    out = ostore[offset:].view(n, S, C + pad)
    if tables is None:
        tables = ops.FcspMap(ymap, xmap, h, w, sp)
    ops.superpixel_pool_fwd(x, tables, out, channels=C)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert (res[..., C:] == SENTINEL).all() and (ostore[:offset] == float(SENTINEL)).all()
    return res[..., :C]


def run_bwd(g, ymap, xmap, sp, h, w, pad=0, offset=0, tables=None):
    n, S, C = g.shape
    gin = np.full((n, S, C + pad), np.nan, np.float32)
    gin[..., :C] = g
    store = torch.empty(gin.size + offset, device='cuda')
    d = store[offset:].view(n, S, C + pad)
    d.copy_(torch.from_numpy(gin))
    ostore = torch.full((n * h * w * (C + pad) + offset,), float(SENTINEL), device='cuda')
    out = ostore[offset:].view(n, h, w, C + pad)
    if tables is None:
        tables = ops.FcspMap(ymap, xmap, h, w, sp)
    ops.superpixel_pool_bwd(d, tables, out, channels=C)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert (res[..., C:] == SENTINEL).all() and (ostore[:offset] == float(SENTINEL)).all()
    return res[..., :C]


@functools.lru_cache(maxsize=None)
def data(name):
    """Tables, inputs and the references of a case, computed once and shared (never written to)."""
    H, W, h, w, sp, align, n, C, pad, offset = CASES[name]
    ymap, xmap = models.fcsp_maps(H, W, h, w, align)
    rng = np.random.default_rng(sorted(CASES).index(name))
    S = (H // sp) * (W // sp)
    feat = rng.standard_normal((n, h, w, C)).astype(np.float32)
    g = rng.standard_normal((n, S, C)).astype(np.float32)
    ifeat = rng.integers(-4096, 4097, (n, h, w, C))
    ig = rng.integers(-4096, 4097, (n, S, C))
    cy, cx = F.counts(ymap, sp, h), F.counts(xmap, sp, w)
    isum_f = np.einsum('Ri,Qj,bijc->bRQc', cy, cx, ifeat).reshape(n, S, C)
    isum_b = np.einsum('Ri,Qj,bRQc->bijc', cy, cx, ig.reshape(n, H // sp, W // sp, C))
    assert np.abs(isum_f).max() <= 2 ** 24 and np.abs(isum_b).max() <= 2 ** 24
    div = np.float32(sp * sp)
    return dict(ymap=ymap, xmap=xmap, sp=sp, h=h, w=w, pad=pad, offset=offset, feat=feat, g=g, ifeat=ifeat.astype(np.float32),
                ig=ig.astype(np.float32), fwd32=F.pool_fwd32(feat, ymap, xmap, sp), bwd32=F.pool_bwd32(g, ymap, xmap, sp, h, w),
                ifwd=isum_f.astype(np.float32) / div, ibwd=isum_b.astype(np.float32) / div, cy=cy, cx=cx)


@pytest.mark.parametrize('name', sorted(CASES))
def test_forward_matches_the_float32_restatement_bit_for_bit(name):
    d = data(name)
    got = run_fwd(d['feat'], d['ymap'], d['xmap'], d['sp'], d['pad'], d['offset'])
    assert bits_equal(got, d['fwd32'])
    got = run_fwd(d['ifeat'], d['ymap'], d['xmap'], d['sp'], d['pad'], d['offset'])
    assert bits_equal(got, d['ifwd'])


@pytest.mark.parametrize('name', sorted(CASES))
def test_backward_matches_the_float32_restatement_bit_for_bit(name):
    d = data(name)
    got = run_bwd(d['g'], d['ymap'], d['xmap'], d['sp'], d['h'], d['w'], d['pad'], d['offset'])
    assert bits_equal(got, d['bwd32'])
    got = run_bwd(d['ig'], d['ymap'], d['xmap'], d['sp'], d['h'], d['w'], d['pad'], d['offset'])
    assert bits_equal(got, d['ibwd'])


def test_cells_without_pixels_get_plus_zero():
    d = data('cells-without-pixels')
    empty = (d['cy'].sum(0)[:, None] * d['cx'].sum(0)[None, :]) == 0
    assert empty.any() and not empty.all()
    got = run_bwd(d['g'], d['ymap'], d['xmap'], d['sp'], d['h'], d['w'])
    assert (got[:, empty].view(np.uint32) == 0).all()                    # +0, not -0, not the sentinel
    assert (got[:, ~empty] != 0).any()


def test_non_finite_values_reach_exactly_their_superpixels():
    d = data('C65-pad3')
    ymap, xmap, sp, h, w = d['ymap'], d['xmap'], d['sp'], d['h'], d['w']
    clean = run_fwd(d['feat'], ymap, xmap, sp, 3)
    feat = d['feat'].copy()
    feat[0, 2, 3, :] = np.nan
    feat[1, 0, 6, :] = np.inf
    got = run_fwd(feat, ymap, xmap, sp, 3)
    weight = np.einsum('Ri,Qj->RQij', d['cy'], d['cx']).reshape(-1, h, w)          # [S, h, w]
    hit = np.zeros(got.shape[:2], bool)
    hit[0] = weight[:, 2, 3] > 0
    hit[1] = weight[:, 0, 6] > 0
    assert hit[0].any() and hit[1].any() and not hit[0].all() and not hit[1].all()
    assert np.isnan(got[0][hit[0]]).all() and (got[1][hit[1]] == np.inf).all()
    assert bits_equal(got[~hit], clean[~hit]) and np.isfinite(got[~hit]).all()
    assert bits_equal(got, F.pool_fwd32(feat, ymap, xmap, sp))
    # the transpose: a NaN in one superpixel's gradient reaches exactly the cells of its window
    cleanb = run_bwd(d['g'], ymap, xmap, sp, h, w, 3)
    g = d['g'].copy()
    s = 4
    g[1, s, :] = np.nan
    gotb = run_bwd(g, ymap, xmap, sp, h, w, 3)
    window = weight[s] > 0
    assert window.any() and not window.all()
    assert np.isnan(gotb[1][window]).all() and np.isfinite(gotb[1][~window]).all() and np.isfinite(gotb[0]).all()
    assert bits_equal(gotb[1][~window], cleanb[1][~window]) and bits_equal(gotb[0], cleanb[0])


@pytest.mark.parametrize('kind', ['out-of-range', 'not-monotone'])
def test_raw_tables_that_fcsp_map_refuses(kind):
    """Entries -1 and h (resp. w): those pixels contribute nothing in either direction, the divisor stays sp * sp, the
    rest is the reference and the run ends clean.  The kernels do not need monotone tables either."""
    d = data('C65-pad3')
    sp, h, w = d['sp'], d['h'], d['w']
    ymap, xmap = d['ymap'].copy(), d['xmap'].copy()
    if kind == 'out-of-range':
        ymap[[0, 5, 13]] = -1
        ymap[[7, 23]] = h
        xmap[[1, 2, 30]] = w
        xmap[[12, 35]] = -1
        xmap[[20]] = 2 ** 31 - 1
        ymap[[14]] = -2 ** 31
    else:
        rng = np.random.default_rng(9)
        ymap, xmap = rng.permutation(ymap), rng.permutation(xmap)
    with pytest.raises(ValueError):
        ops.FcspMap(ymap, xmap, h, w, sp)
    raw = (torch.from_numpy(ymap).cuda(), torch.from_numpy(xmap).cuda(), sp)
    got = run_fwd(d['feat'], ymap, xmap, sp, 3, tables=raw)
    assert bits_equal(got, F.pool_fwd32(d['feat'], ymap, xmap, sp)) and np.isfinite(got).all()
    gotb = run_bwd(d['g'], ymap, xmap, sp, h, w, 3, tables=raw)
    assert bits_equal(gotb, F.pool_bwd32(d['g'], ymap, xmap, sp, h, w)) and np.isfinite(gotb).all()
    if kind == 'out-of-range':
        assert (F.counts(ymap, sp, h).sum(1) < sp).any() and not bits_equal(got, d['fwd32'])
    torch.cuda.synchronize()


def test_two_runs_give_identical_bits():
    d = data('model-centre')
    a = run_fwd(d['feat'], d['ymap'], d['xmap'], d['sp'])
    b = run_fwd(d['feat'], d['ymap'], d['xmap'], d['sp'])
    assert bits_equal(a, b)
    a = run_bwd(d['g'], d['ymap'], d['xmap'], d['sp'], d['h'], d['w'])
    b = run_bwd(d['g'], d['ymap'], d['xmap'], d['sp'], d['h'], d['w'])
    assert bits_equal(a, b)


def test_wrapper_refuses_what_does_not_fit():
    d = data('C3-pad3')
    m = ops.FcspMap(d['ymap'], d['xmap'], d['h'], d['w'], d['sp'])
    x = torch.zeros((2, d['h'], d['w'], 3), device='cuda')
    with pytest.raises(ValueError):
        ops.superpixel_pool_fwd(x[:, :-1].contiguous(), m)                # a map of another size
    with pytest.raises(ValueError):
        ops.superpixel_pool_fwd(x, m, torch.zeros((2, m.S + 1, 3), device='cuda'))
    with pytest.raises(ValueError):
        ops.superpixel_pool_fwd(x, m, channels=4)
    with pytest.raises(TypeError):
        ops.superpixel_pool_fwd(x.double(), m)
    assert ops.superpixel_pool_fwd(x, m).shape == (2, m.S, 3)
