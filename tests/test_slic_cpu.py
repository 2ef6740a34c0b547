"""The host references of the SLIC entry points (tests/slic_ref.py) on their own, without a GPU: the properties the
header states hold for the references, the float32 restatements stay within their derived bounds of float64, the pooling
on grid labels is tests/fcsp_ref.py's, and the inputs the GPU tests use meet the near-tie condition their assignment
check relies on."""
import functools

import numpy as np
import pytest
import torch

import fcsp_ref
import slic_ref as S

SMALL = ['12x16', '8x8', '15x20']


@functools.lru_cache(maxsize=None)
def segmented(name, iters=3):
    n, H, W, sp = S.CASES[name]
    return S.segment32(S.image(name), sp, iters, S.COMPACTNESS)


@pytest.mark.parametrize('name', SMALL)
@pytest.mark.parametrize('iters', [0, 1, 5])
def test_a_constant_image_keeps_the_grid(name, iters):
    n, H, W, sp = S.CASES[name]
    x = np.full((n, H, W, 3), 0.3, np.float32)
    labels, centres, cnt = S.segment32(x, sp, iters, S.COMPACTNESS)
    assert (labels == S.grid_labels(n, H, W, sp)).all() and (cnt == sp * sp).all()
    rows, cols, _ = S.geometry(H, W, sp)
    want = np.stack(np.meshgrid(np.arange(rows) * sp + (sp - 1) / 2, np.arange(cols) * sp + (sp - 1) / 2, indexing='ij'), -1)
    assert (centres[..., :2] == want.reshape(1, -1, 2)).all()


@pytest.mark.parametrize('name', SMALL + ['240x320-40'])
def test_a_segmentation_keeps_candidates_anchors_and_every_pixel(name):
    n, H, W, sp = S.CASES[name]
    labels, centres, cnt = segmented(name)
    grid = S.grid_labels(n, H, W, sp)
    assert (labels != grid).any()                                             # the images do move pixels
    assert S.counts_mask(labels, sp).all()                                    # every label lies in N(y, x)
    for b, y, x in [(0, 0, 0), (0, H - 1, W - 1), (0, H // 2, W // 2), (0, 0, W // 2)]:
        assert labels[b, y, x] in S.candidates(y, x, H, W, sp)
    assert (labels[:, S.anchors(H, W, sp)] == grid[:, S.anchors(H, W, sp)]).all()
    assert (cnt > 0).all() and (cnt.sum(1) == H * W).all()
    assert np.isfinite(centres).all()
    assert (S.segment32(S.image(name), sp, 0, S.COMPACTNESS)[0] == grid).all()


def test_candidate_sets_have_four_six_and_nine_members():
    n, H, W, sp = S.CASES['12x16']
    sizes = {len(S.candidates(y, x, H, W, sp)) for y in range(H) for x in range(W)}
    assert sizes == {4, 6, 9}
    assert S.candidates(5, 6, H, W, sp) == [0, 1, 2, 4, 5, 6, 8, 9, 10]
    n, H, W, sp = S.CASES['8x8']
    assert {len(S.candidates(y, x, H, W, sp)) for y in range(H) for x in range(W)} == {4}


@pytest.mark.parametrize('name', ['12x16', '15x20'])              # 3 x 4 grids: a 2 x 2 grid has no far superpixel
def test_label_contract_of_the_reference(name):
    """Foreign, negative, too large and far labels count nowhere; the float32 means stay within (count + 1) 2^-24."""
    n, H, W, sp = S.CASES[name]
    labels = segmented(name)[0].copy()
    total = S.geometry(H, W, sp)[2]
    labels[0, 0, 0], labels[0, 1, 1], labels[0, 2, 2] = -1, total, total - 1   # (2, 2) is far from the last superpixel
    labels[0, H - 1, W - 1] = 0
    cnt = S.label_count(labels, sp)
    assert cnt[0].sum() == H * W - 4 and (cnt[1:].sum(1) == H * W).all()
    x = S.image(name)
    c32, m32 = S.label_mean32(x, labels, sp)
    c64, m64 = S.label_mean64(x, labels, sp)
    assert (c32 == c64).all() and (S.label_hist(x, labels, sp).sum(-1) == c64).all()
    assert (np.abs(m32 - m64) <= (c64[..., None] + 1) * S.U * np.abs(m64)).all()
    ce32, _ = S.update32(x, labels, sp)
    ce64, _ = S.update64(x, labels, sp)
    assert (ce32[..., :2] == ce64[..., :2].astype(np.float32)).all()         # one rounding of the exact mean
    assert (ce32[..., 2:].view(np.uint32) == m32.view(np.uint32)).all()


@pytest.mark.parametrize('name', sorted(S.CASES))
def test_the_gpu_tests_inputs_meet_the_near_tie_condition(name):
    """At most 1 % of the pixels are undecided (the two best float64 distances within 64 * 2^-24 of the larger), for the
    perturbed centres the assignment test uses and for every iteration of the reference's own trajectory."""
    n, H, W, sp = S.CASES[name]
    x = S.image(name)
    labels, second, decided = S.assign64(x, S.perturbed_centres(name), sp, S.COMPACTNESS)
    assert (~decided).sum() <= 0.01 * decided.size
    got = S.assign32(x, S.perturbed_centres(name), sp, S.COMPACTNESS)
    assert (got[decided] == labels[decided]).all() and ((got == labels) | (got == second)).all()
    if name in SMALL:
        lab = S.grid_labels(n, H, W, sp)
        ce, _ = S.update32(x, lab, sp)
        for _ in range(3):
            _, _, decided = S.assign64(x, ce, sp, S.COMPACTNESS)
            assert (~decided).sum() <= 0.01 * decided.size
            lab = S.assign32(x, ce, sp, S.COMPACTNESS)
            ce, _ = S.update32(x, lab, sp, ce)


def test_ties_nan_centres_and_the_anchor_in_the_reference():
    n, H, W, sp = S.CASES['12x16']
    x = S.image('12x16')
    total = S.geometry(H, W, sp)[2]
    same = np.tile(np.array([5.5, 7.5, 0.5, 0.5, 0.5], np.float32), (n, total, 1))
    labels = S.assign32(x, same, sp, S.COMPACTNESS)                           # every candidate at the same distance
    grid = S.grid_labels(n, H, W, sp)
    lowest = np.array([[S.candidates(y, xx, H, W, sp)[0] for xx in range(W)] for y in range(H)])
    assert (labels == np.where(S.anchors(H, W, sp), grid, lowest)).all()
    nan = np.full_like(same, np.nan)
    assert (S.assign32(x, nan, sp, S.COMPACTNESS) == grid).all()              # none left: the home
    ce = S.perturbed_centres('12x16')
    ce[:, 5] = np.nan
    assert not (S.assign32(x, ce, sp, S.COMPACTNESS) == 5)[~np.broadcast_to(S.anchors(H, W, sp), grid.shape)].any()
    assert (S.assign32(x, ce, sp, S.COMPACTNESS)[:, S.anchors(H, W, sp)] == grid[:, S.anchors(H, W, sp)]).all()


def tables(H, W, h, w):
    return (np.arange(H) * h // H).astype(np.int32), (np.arange(W) * w // W).astype(np.int32)


def test_pooling_on_grid_labels_is_the_grid_pooling_bit_for_bit():
    n, H, W, sp = S.CASES['12x16']
    h, w, C = 5, 7, 6
    ymap, xmap = tables(H, W, h, w)
    rng = np.random.default_rng(5)
    feat = rng.standard_normal((n, h, w, C)).astype(np.float32)
    g = rng.standard_normal((n, S.geometry(H, W, sp)[2], C)).astype(np.float32)
    cnt = S.pool_counts(S.grid_labels(n, H, W, sp), ymap, xmap, sp, h, w)
    count = np.full(cnt.shape[:2], sp * sp)
    assert (cnt[0] == np.einsum('Ri,Qj->RQij', fcsp_ref.counts(ymap, sp, h), fcsp_ref.counts(xmap, sp, w)).reshape(-1, h, w)).all()
    a, b = S.pool_fwd32(feat, cnt, count), fcsp_ref.pool_fwd32(feat, ymap, xmap, sp)
    assert (a.view(np.uint32) == b.view(np.uint32)).all()
    assert np.allclose(S.pool_bwd64(g, cnt, count), fcsp_ref.pool_bwd64(g, ymap, xmap, sp, h, w), rtol=1e-13, atol=0)


@pytest.mark.parametrize('name', SMALL)
def test_the_pool_pair_is_adjoint_in_float64(name):
    n, H, W, sp = S.CASES[name]
    h, w, C = 4, 5, 3
    ymap, xmap = tables(H, W, h, w)
    ymap[1] = -1
    xmap[2] = w
    labels, _, count = segmented(name)
    labels = labels.copy()
    labels[0, 0, 0] = -7
    count = count.copy()
    count[0, 1] = 0                                                            # a superpixel the caller declares empty
    cnt = S.pool_counts(labels, ymap, xmap, sp, h, w)
    rng = np.random.default_rng(6)
    f = rng.standard_normal((n, h, w, C))
    g = rng.standard_normal((n, cnt.shape[1], C))
    lhs, rhs = (S.pool_fwd64(f, cnt, count) * g).sum(), (f * S.pool_bwd64(g, cnt, count)).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1)
    assert (S.pool_fwd64(f, cnt, count)[0, 1] == 0).all()
    e = np.abs(S.pool_fwd32(f, cnt, count) - S.pool_fwd64(f.astype(np.float32), cnt, count)).max()
    assert 0 < e < 1e-5
    e = np.abs(S.pool_bwd32(g, cnt, count) - S.pool_bwd64(g.astype(np.float32), cnt, count)).max()
    assert 0 < e < 1e-5


def test_the_similarity_reference_matches_torch():
    name = '12x16'
    n, H, W, sp = S.CASES[name]
    x = S.image(name)
    labels, _, count = segmented(name)
    _, mean3 = S.label_mean64(x, labels, sp)
    hist = S.label_hist(x, labels, sp)
    rows, cols, total = S.geometry(H, W, sp)
    left = np.array([s for s in range(total) if s % cols < cols - 1] + [s for s in range(total - cols)])
    right = np.array([s + 1 for s in range(total) if s % cols < cols - 1] + [s + cols for s in range(total - cols)])
    dw, db, gamma = np.array([0.7, 0.4]), np.array([0.05]), 1.5
    sims, r = S.pair_similarity64(mean3, hist, count, left, right, dw, db, gamma)
    m, f = torch.from_numpy(mean3), torch.from_numpy(hist / count[..., None])
    t0 = torch.exp(-gamma * torch.linalg.vector_norm(m[:, left] - m[:, right], dim=-1))
    t1 = torch.exp(-gamma * torch.linalg.vector_norm(f[:, left] - f[:, right], dim=-1))
    assert np.allclose(sims[..., 0], t0.numpy(), rtol=1e-12) and np.allclose(sims[..., 1], t1.numpy(), rtol=1e-12)
    assert np.allclose(r, (t0 * dw[0] + t1 * dw[1] + db[0]).numpy(), rtol=1e-12)
    assert (sims > 0).all() and (sims <= 1).all() and sims[..., 1].min() > 0.1      # not the reference's "essentially 0"
    s32, r32 = S.pair_similarity32(mean3, hist, count, left, right, dw, db, gamma)
    assert np.abs(s32 - sims).max() < 1e-6 and np.abs(r32 - r).max() < 1e-6
    bad_l = left.copy()
    bad_l[3] = total
    sims_b, r_b = S.pair_similarity64(mean3, hist, count, bad_l, right, dw, db, gamma)
    assert np.isnan(sims_b[:, 3]).all() and np.isnan(r_b[:, 3]).all() and np.isfinite(np.delete(r_b, 3, 1)).all()
