"""Host references of the SLIC entry points (include/a3d_slic.h): segmentation on the 3 x 3 candidate clusters of a pixel's
home cell, and the label-driven mean, histogram, pair similarities and feature pooling.

TEST INFRASTRUCTURE ONLY.  Every entry point is stated twice: in float64 from the definitions, and in float32 in the order
the header gives the kernels (the lanes' partial sums over the row-major window, folded 128 .. 1; every operation rounded
on its own).  Nothing here is derived from the kernels' code."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32
F = np.float32
LANES = 256


def geometry(H, W, sp):
    assert H % sp == 0 and W % sp == 0
    return H // sp, W // sp, (H // sp) * (W // sp)


def grid_labels(n, H, W, sp):
    rows, cols, _ = geometry(H, W, sp)
    lab = (np.arange(H)[:, None] // sp) * cols + np.arange(W)[None, :] // sp
    return np.broadcast_to(lab.astype(np.int32), (n, H, W)).copy()


def candidates(y, x, H, W, sp):
    """N(y, x): the superpixels (R + dr, C + dc) inside the grid, ascending."""
    rows, cols, _ = geometry(H, W, sp)
    R, C = y // sp, x // sp
    return [(R + dr) * cols + C + dc for dr in (-1, 0, 1) for dc in (-1, 0, 1) if 0 <= R + dr < rows and 0 <= C + dc < cols]


def counts_mask(labels, sp):
    """[n,H,W] bool: the pixel's label is a superpixel among its candidates (the label contract)."""
    n, H, W = labels.shape
    rows, cols, S = geometry(H, W, sp)
    lab = labels.astype(np.int64)
    ok = (lab >= 0) & (lab < S)
    safe = np.where(ok, lab, 0)
    R, C = np.arange(H)[None, :, None] // sp, np.arange(W)[None, None, :] // sp
    return ok & (np.abs(safe // cols - R) <= 1) & (np.abs(safe % cols - C) <= 1)


def anchors(H, W, sp):
    """[H,W] bool: the pixel (R sp + sp // 2, C sp + sp // 2) of every cell."""
    return ((np.arange(H) % sp == sp // 2)[:, None]) & ((np.arange(W) % sp == sp // 2)[None, :])


def window(s, H, W, sp):
    rows, cols, _ = geometry(H, W, sp)
    R, C = s // cols, s % cols
    return max((R - 1) * sp, 0), min((R + 2) * sp, H), max((C - 1) * sp, 0), min((C + 2) * sp, W)


# ----------------------------------------------------------------------------------------------------------------------
# label statistics
# ----------------------------------------------------------------------------------------------------------------------
def label_count(labels, sp):
    n, H, W = labels.shape
    S = geometry(H, W, sp)[2]
    m = counts_mask(labels, sp)
    out = np.zeros((n, S), np.int64)
    for b in range(n):
        out[b] = np.bincount(labels[b][m[b]].astype(np.int64), minlength=S)
    return out


def label_sum64(v, labels, sp):
    """v [n,H,W,c] -> (count [n,S] int64, sums [n,S,c] float64) over the pixels that count."""
    n, H, W = labels.shape
    S = geometry(H, W, sp)[2]
    m = counts_mask(labels, sp)
    v = np.asarray(v, np.float64)
    sums = np.zeros((n, S, v.shape[3]))
    for b in range(n):
        np.add.at(sums[b], labels[b][m[b]].astype(np.int64), v[b][m[b]])
    return label_count(labels, sp), sums


def label_mean64(v, labels, sp):
    cnt, sums = label_sum64(v, labels, sp)
    with np.errstate(invalid='ignore', divide='ignore'):
        return cnt, np.where(cnt[..., None] > 0, sums / cnt[..., None], np.nan)


def fold(p):
    """p [256, ...] float32 -> the header's sum of a block."""
    p = np.array(p, F)
    k = LANES // 2
    while k:
        p[:k] = p[:k] + p[k:2 * k]
        k //= 2
    return p[0]


def block_sum32(terms, mask):
    """terms [Q, c] float32 in window order, mask [Q]: lane t adds the terms t, t + 256, ... that count, then the fold."""
    Q, c = terms.shape
    pad = (-Q) % LANES
    t = np.concatenate([np.where(mask[:, None], terms, F(0)).astype(F), np.zeros((pad, c), F)]).reshape(-1, LANES, c)
    p = np.zeros((LANES, c), F)
    for row in t:
        p = p + row
    return fold(p)


def label_mean32(v, labels, sp):
    """a3ds_label_mean's arithmetic: (count [n,S] int32, mean [n,S,c] float32)."""
    v = np.asarray(v, F)
    n, H, W, c = v.shape
    S = geometry(H, W, sp)[2]
    cnt = label_count(labels, sp)
    mean = np.full((n, S, c), np.nan, F)
    for b in range(n):
        for s in range(S):
            y0, y1, x0, x1 = window(s, H, W, sp)
            if cnt[b, s]:
                mean[b, s] = block_sum32(v[b, y0:y1, x0:x1].reshape(-1, c), labels[b, y0:y1, x0:x1].reshape(-1) == s) / F(cnt[b, s])
    return cnt.astype(np.int32), mean


def colour_bin32(px):
    """color_histogram's bin of RGB pixels [..., 3] in float32 (src/models.py:95-100)."""
    px = np.asarray(px, F)
    v = (px[..., 0] * F(16777216) + px[..., 1] * F(65536)) + px[..., 2] * F(256)
    scaled = v / F(16777216)
    return np.clip(np.floor(F(256) * scaled), 0, 255).astype(np.int64)


def label_hist(x, labels, sp):
    """[n,S,256] int64."""
    n, H, W = labels.shape
    S = geometry(H, W, sp)[2]
    m = counts_mask(labels, sp)
    bins = colour_bin32(x)
    out = np.zeros((n, S, 256), np.int64)
    for b in range(n):
        np.add.at(out[b], (labels[b][m[b]].astype(np.int64), bins[b][m[b]]), 1)
    return out


def coords(n, H, W):
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    return np.broadcast_to(np.stack([yy, xx], -1)[None], (n, H, W, 2))


def update64(x, labels, sp, centres=None):
    """(centres [n,S,5] float64, count); a superpixel without pixels keeps the row of `centres` (NaN without it)."""
    n, H, W = labels.shape
    cnt, mean = label_mean64(np.concatenate([coords(n, H, W), np.asarray(x, np.float64)], -1), labels, sp)
    if centres is not None:
        mean = np.where(cnt[..., None] > 0, mean, np.asarray(centres, np.float64))
    return mean, cnt


def update32(x, labels, sp, centres=None):
    """a3ds_slic_update's arithmetic: exact integer coordinate sums, one division each; the colours are label_mean32's."""
    n, H, W = labels.shape
    cnt, col = label_mean32(x, labels, sp)
    _, csum = label_sum64(coords(n, H, W), labels, sp)
    assert csum.max() < 2 ** 24
    with np.errstate(invalid='ignore', divide='ignore'):
        pos = csum.astype(F) / cnt[..., None].astype(F)
    out = np.concatenate([pos, col], -1).astype(F)
    if centres is not None:
        out = np.where(cnt[..., None] > 0, out, np.asarray(centres, F))
    return out, cnt


# ----------------------------------------------------------------------------------------------------------------------
# assignment
# ----------------------------------------------------------------------------------------------------------------------
def distances(x, centres, sp, compactness, dtype):
    """D [9, n, H, W] (inf-free: NaN where the candidate is outside the grid), index [9, n, H, W] (-1 outside): the nine
    (dr, dc) in ascending superpixel index, in `dtype` arithmetic with the header's operation order."""
    x = np.asarray(x, dtype)
    n, H, W, _ = x.shape
    rows, cols, S = geometry(H, W, sp)
    ce = np.asarray(centres, dtype)
    q = dtype(compactness) / dtype(sp)
    wgt = dtype(q * q)
    R, C = np.arange(H)[:, None] // sp, np.arange(W)[None, :] // sp
    yy, xx = np.arange(H, dtype=dtype)[None, :, None], np.arange(W, dtype=dtype)[None, None, :]
    D, K = [], []
    with np.errstate(invalid='ignore', over='ignore'):
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                Rk, Ck = R + dr, C + dc
                inside = np.broadcast_to((Rk >= 0) & (Rk < rows) & (Ck >= 0) & (Ck < cols), (H, W))
                k = np.where(inside, Rk * cols + Ck, 0)
                c = ce[:, k]                                                  # [n,H,W,5]
                d0, d1, d2 = x[..., 0] - c[..., 2], x[..., 1] - c[..., 3], x[..., 2] - c[..., 4]
                col = (d0 * d0 + d1 * d1) + d2 * d2
                dy, dx = yy - c[..., 0], xx - c[..., 1]
                d = col + wgt * (dy * dy + dx * dx)
                D.append(np.where(inside[None], d, np.nan))
                K.append(np.broadcast_to(np.where(inside, k, -1)[None], (n, H, W)))
    return np.stack(D), np.stack(K)


def pick(D, K, H, W, sp):
    """The label rule on distances: smallest D, ties to the lowest index, NaN skipped, home without any; anchors home."""
    n = D.shape[1]
    home = grid_labels(n, H, W, sp)
    best = home.copy()
    best_d = np.full(D.shape[1:], np.inf, D.dtype)
    found = np.zeros(D.shape[1:], bool)
    for d, k in zip(D, K):
        take = ~np.isnan(d) & (~found | (d < best_d))
        best, best_d, found = np.where(take, k, best), np.where(take, d, best_d), found | take
    return np.where(anchors(H, W, sp)[None], home, best).astype(np.int32)


def assign32(x, centres, sp, compactness):
    n, H, W, _ = x.shape
    return pick(*distances(x, centres, sp, compactness, F), H, W, sp)


def assign64(x, centres, sp, compactness, rel=64 * U):
    """(labels, second, decided): float64 labels; the runner-up candidate (-1 without one); decided [n,H,W] bool: the two
    best D differ by more than `rel` of the larger (anchors and pixels with one live candidate are decided)."""
    n, H, W, _ = x.shape
    D, K = distances(x, centres, sp, compactness, np.float64)
    labels = pick(D, K, H, W, sp)
    Dm = np.where(np.isnan(D), np.inf, D)
    order = np.argsort(Dm, axis=0, kind='stable')
    d_sorted = np.take_along_axis(Dm, order, 0)
    k_sorted = np.take_along_axis(K, order, 0)
    second = np.where(np.isfinite(d_sorted[1]), k_sorted[1], -1)
    decided = ~np.isfinite(d_sorted[1]) | (d_sorted[1] - d_sorted[0] > rel * d_sorted[1]) | anchors(H, W, sp)[None]
    return labels, second.astype(np.int32), decided


def segment32(x, sp, iters, compactness):
    """a3ds_slic_segment in the float32 restatements: (labels, centres, count)."""
    n, H, W, _ = x.shape
    labels = grid_labels(n, H, W, sp)
    centres, cnt = update32(x, labels, sp)
    for _ in range(iters):
        labels = assign32(x, centres, sp, compactness)
        centres, cnt = update32(x, labels, sp, centres)
    return labels, centres, cnt


# ----------------------------------------------------------------------------------------------------------------------
# pair similarities
# ----------------------------------------------------------------------------------------------------------------------
def pair_similarity64(mean3, hist, count, left, right, dw, db, gamma):
    """(sims [n,Q,2], r [n,Q]) float64; NaN for a pair with an index outside [0, S)."""
    mean3, hist = np.asarray(mean3, np.float64), np.asarray(hist, np.float64)
    n, S, _ = mean3.shape
    left, right = np.asarray(left, np.int64), np.asarray(right, np.int64)
    ok = (left >= 0) & (left < S) & (right >= 0) & (right < S)
    l, r = np.where(ok, left, 0), np.where(ok, right, 0)
    with np.errstate(invalid='ignore', divide='ignore'):
        freq = hist / np.asarray(count, np.float64)[..., None]
        s0 = np.exp(-gamma * np.sqrt(((mean3[:, l] - mean3[:, r]) ** 2).sum(-1)))
        s1 = np.exp(-gamma * np.sqrt(((freq[:, l] - freq[:, r]) ** 2).sum(-1)))
    sims = np.where(ok[None, :, None], np.stack([s0, s1], -1), np.nan)
    dw, db = np.asarray(dw, np.float64).reshape(-1), np.asarray(db, np.float64).reshape(-1)
    return sims, (sims[..., 0] * dw[0] + sims[..., 1] * dw[1]) + db[0]


def pair_similarity32(mean3, hist, count, left, right, dw, db, gamma):
    """a3ds_pair_similarity's arithmetic (numpy's float32 exp and sqrt standing for expf and sqrtf)."""
    mean3, hist = np.asarray(mean3, F), np.asarray(hist, F)
    n, S, _ = mean3.shape
    left, right = np.asarray(left, np.int64), np.asarray(right, np.int64)
    ok = (left >= 0) & (left < S) & (right >= 0) & (right < S)
    l, r = np.where(ok, left, 0), np.where(ok, right, 0)
    g = F(gamma)
    with np.errstate(invalid='ignore', divide='ignore'):
        freq = hist / np.asarray(count).astype(F)[..., None]
        e = mean3[:, l] - mean3[:, r]
        sc = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
        f = freq[:, l] - freq[:, r]                                           # [n,Q,256]
        sh = fold(np.moveaxis(f * f, -1, 0))
        s0, s1 = np.exp(-g * np.sqrt(sc)), np.exp(-g * np.sqrt(sh))
    sims = np.where(ok[None, :, None], np.stack([s0, s1], -1), F(np.nan)).astype(F)
    dw, db = np.asarray(dw, F).reshape(-1), np.asarray(db, F).reshape(-1)
    return sims, ((sims[..., 0] * dw[0] + sims[..., 1] * dw[1]) + db[0]).astype(F)


# ----------------------------------------------------------------------------------------------------------------------
# label pooling
# ----------------------------------------------------------------------------------------------------------------------
def pool_counts(labels, ymap, xmap, sp, h, w):
    """cnt [n,S,h,w] int64: the pixels that count for s with ymap[y] = i, xmap[x] = j, both in range."""
    n, H, W = labels.shape
    S = geometry(H, W, sp)[2]
    ymap, xmap = np.asarray(ymap, np.int64), np.asarray(xmap, np.int64)
    m = counts_mask(labels, sp) & ((ymap >= 0) & (ymap < h))[None, :, None] & ((xmap >= 0) & (xmap < w))[None, None, :]
    cell_i = np.broadcast_to(ymap[None, :, None], labels.shape)
    cell_j = np.broadcast_to(xmap[None, None, :], labels.shape)
    out = np.zeros((n, S, h, w), np.int64)
    for b in range(n):
        np.add.at(out[b], (labels[b][m[b]].astype(np.int64), cell_i[b][m[b]], cell_j[b][m[b]]), 1)
    return out


def _inv(count):
    count = np.asarray(count, np.float64)
    with np.errstate(divide='ignore'):
        return np.where(count > 0, 1.0 / count, 0.0)


def pool_fwd64(feat, cnt, count):
    """feat [n,h,w,C], cnt [n,S,h,w], count [n,S] -> [n,S,C] float64 (finite data); 0 where count <= 0."""
    return np.einsum('bsij,bijc->bsc', cnt.astype(np.float64), np.asarray(feat, np.float64)) * _inv(count)[..., None]


def pool_bwd64(dpooled, cnt, count):
    """dpooled [n,S,C] -> [n,h,w,C] float64, the transpose of pool_fwd64."""
    return np.einsum('bsij,bsc->bijc', cnt.astype(np.float64), np.asarray(dpooled, np.float64) * _inv(count)[..., None])


def pool_fwd32(feat, cnt, count):
    """The forward kernel's arithmetic: cells ascending, zero counts skipped, one division; +0 where count <= 0."""
    feat = np.asarray(feat, F)
    n, h, w, C = feat.shape
    S = cnt.shape[1]
    out = np.zeros((n, S, C), F)
    flat, cf = feat.reshape(n, h * w, C), cnt.reshape(n, S, h * w)
    with np.errstate(invalid='ignore', over='ignore'):
        for b in range(n):
            for s in range(S):
                if count[b, s] <= 0:
                    continue
                acc = np.zeros(C, F)
                for cell in np.flatnonzero(cf[b, s]):
                    acc = acc + F(cf[b, s, cell]) * flat[b, cell]
                out[b, s] = acc / F(count[b, s])
    return out


def pool_bwd32(dpooled, cnt, count):
    """The backward kernel's arithmetic: superpixels ascending, zero counts skipped, one division per term."""
    dpooled = np.asarray(dpooled, F)
    n, S, C = dpooled.shape
    h, w = cnt.shape[2:]
    out = np.zeros((n, h * w, C), F)
    cf = cnt.reshape(n, S, h * w)
    with np.errstate(invalid='ignore', over='ignore'):
        for b in range(n):
            for cell in range(h * w):
                acc = np.zeros(C, F)
                for s in np.flatnonzero(cf[b, :, cell]):
                    if count[b, s] > 0:
                        acc = acc + (F(cf[b, s, cell]) * dpooled[b, s]) / F(count[b, s])
                out[b, cell] = acc
    return out.reshape(n, h, w, C)


# ----------------------------------------------------------------------------------------------------------------------
# the inputs the CPU and the GPU tests share
# ----------------------------------------------------------------------------------------------------------------------
COMPACTNESS = 0.1
# name: (n, H, W, sp)
CASES = {'12x16': (2, 12, 16, 4),            # 3 x 4 grid: corner, edge and interior homes, candidate sets of 4, 6 and 9
         '8x8': (1, 8, 8, 4),                # all corners
         '15x20': (2, 15, 20, 5),            # odd sp: the block centroid is a pixel
         '240x320-10': (1, 240, 320, 10),    # the model's image at its finest and coarsest grid
         '240x320-40': (1, 240, 320, 40)}


def image(name):
    """[n,H,W,3] float32 in [0, 1]: a few flat regions with straight borders that ignore the grid, plus noise."""
    n, H, W, sp = CASES[name]
    rng = np.random.default_rng(100 + sorted(CASES).index(name))
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    out = np.empty((n, H, W, 3))
    for b in range(n):
        region = np.zeros((H, W), np.int64)
        for k in range(4):
            a, c = rng.normal(size=2)
            region += (a * (yy - rng.uniform(0, H)) + c * (xx - rng.uniform(0, W)) > 0) << k
        out[b] = rng.uniform(0.1, 0.9, (16, 3))[region] + rng.uniform(-0.1, 0.1, (H, W, 3))
    return out.astype(F)


def perturbed_centres(name):
    """The grid's centres, positions moved by up to one pixel: [n,S,5] float32."""
    n, H, W, sp = CASES[name]
    rng = np.random.default_rng(200 + sorted(CASES).index(name))
    ce, _ = update64(image(name), grid_labels(n, H, W, sp), sp)
    ce[..., :2] += rng.uniform(-1, 1, ce[..., :2].shape)
    return ce.astype(F)
