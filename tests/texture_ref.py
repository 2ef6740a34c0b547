"""References of the texture kernels (include/a3d_texture.h: a3dt_superpixel_lbp_hist, a3dt_pair_similarity3) in numpy,
for any image size (h, w) and superpixel edge sp (tests/test_texture_cpu.py, tests/test_gpu_texture.py,
tests/test_gpu_texture_train.py).  The first two similarities, the block sums and the cases are dcnf_pair_ref's.

grey(x)                  [n, h, w, 3] float32 -> [n, h, w]: ((x0 + x1) + x2) / 3, each operation rounded on its own
lbp_codes(x)             [n, h, w] uint8: bit k is set iff the grey value at offset k, clamped into the image, is >= the
                         pixel's own; k = 0 .. 7 are (-1,-1) (-1,0) (-1,+1) (0,+1) (+1,+1) (+1,0) (+1,-1) (0,-1) as (dy, dx).
                         Vectorised over an edge-padded grey image (edge padding by one pixel IS the clamp).
lbp_codes_loop(x)        the same by a literal double loop over the pixels, for the comparison of the two
lbp_histogram(x, sp)     counts of the raw codes per superpixel [n, P, 256] (float32, exact)
similarity3_64 / 32      (sims [n, Q, 3], r [n, Q]) from an image, its two histograms, pair lists, the 3 -> 1 dense layer and
                         gamma.  sims[..., :2] are dcnf_pair_ref's; sims[..., 2] = exp(-gamma (sqrt(S_t) / (sp sp))) with
                         S_t = sum_bins (lbp_l - lbp_r)^2; r = ((s0 w0 + s1 w1) + s2 w2) + b.  The float32 form sums as
                         the kernel does (dcnf_pair_ref._block_sum32).
texture_bound(...)       per (image, pair) relative bound of sims[..., 2] against float64

The texture similarity needs no measurement.  The counts are integers and S_t <= 2 (sp sp)^2 < 2^24 for sp <= 53 is exact
in float32 in any order.  What remains is expf(-gamma * (sqrtf(S_t) / (float)(sp sp))): sqrtf within 1 ulp (2u, u = 2^-24),
the division and the product rounded once each (u, u), so the argument t carries a relative error of at most 4u, which
expf turns into |t| 4u of its result; expf's own error is at most 1 ulp (2u).  texture_bound = (4 |t| + 3) u, the last u
for the second-order terms: dcnf_pair_ref.hist_bound with one more rounding.

r is held like dcnf_pair_ref's: over SHAPES x GAMMAS x pair lists of length 1 and 100 on the three images of
dcnf_pair_ref.image (the cases of tests/test_gpu_texture.py; measured() below) the float32 form lies from float64, per
image and ||.||inf-relative, by at most
                                                         measured     bound = 8 x    kernel on an MI355X reached
  r (three similarities)                                 1.30e-07     1.1e-06        9.22e-08
and the texture similarity's kernel reached 0.258 of its derived bound at the worst.
"""
import numpy as np

import dcnf_pair_ref as P
from crf_loss_ref import F, U

# 8 x the measured worst, rounded up to two digits
R3_BOUND = 1.1e-06

# (dy, dx) of bit k
OFFSETS = [(-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1)]
MAX_SP = 53


def grey(x):
    x = np.ascontiguousarray(x, F)
    assert x.shape[-1] == 3
    with np.errstate(all='ignore'):
        return ((x[..., 0] + x[..., 1]) + x[..., 2]) / F(3)


def lbp_codes(x):
    g = grey(x)
    n, h, w = g.shape
    pad = np.pad(g, ((0, 0), (1, 1), (1, 1)), mode='edge')
    code = np.zeros((n, h, w), np.uint8)
    with np.errstate(invalid='ignore'):
        for k, (dy, dx) in enumerate(OFFSETS):
            code |= (pad[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w] >= g).astype(np.uint8) << k
    return code


def lbp_codes_loop(x):
    g = grey(x)
    n, h, w = g.shape
    code = np.zeros((n, h, w), np.uint8)
    with np.errstate(invalid='ignore'):
        for b in range(n):
            for y in range(h):
                for xx in range(w):
                    c = 0
                    for k, (dy, dx) in enumerate(OFFSETS):
                        if g[b, min(max(y + dy, 0), h - 1), min(max(xx + dx, 0), w - 1)] >= g[b, y, xx]:
                            c |= 1 << k
                    code[b, y, xx] = c
    return code


def lbp_histogram(x, sp, codes=None):
    code = lbp_codes(x) if codes is None else codes
    idx = P.blocks(code[..., None].astype(np.int64), sp)[..., 0]              # [n, P, sp * sp]
    n, nsp, m = idx.shape
    flat = (np.arange(n * nsp)[:, None] * 256 + idx.reshape(n * nsp, m)).ravel()
    return np.bincount(flat, minlength=n * nsp * 256).reshape(n, nsp, 256).astype(F)


def s_t(lbp, left, right):
    """The exact S_t [n, Q] in float64."""
    h = np.asarray(lbp, np.float64)
    d = h[:, np.asarray(left, np.int64)] - h[:, np.asarray(right, np.int64)]
    return (d * d).sum(axis=2)


def _similarity3(x, sp, hist, lbp, left, right, dense_w, dense_b, gamma, dt):
    dw, db = np.asarray(dense_w, dt).ravel(), np.asarray(dense_b, dt).ravel()
    assert dw.size == 3
    sims2, _, _ = P._similarity(x, sp, hist, left, right, dw[:2], db, gamma, dt)
    left, right = np.asarray(left, np.int64), np.asarray(right, np.int64)
    d = np.asarray(lbp, dt)[:, left] - np.asarray(lbp, dt)[:, right]
    with np.errstate(under='ignore'):
        st = P._block_sum32(d * d) if dt is F else (d * d).sum(axis=2)
        tdiff = np.exp(-dt(gamma) * (np.sqrt(st) / dt(sp * sp)))
        cdiff, hdiff = sims2[..., 0], sims2[..., 1]
        r = ((cdiff * dw[0] + hdiff * dw[1]) + tdiff * dw[2]) + db[0]
    return np.stack([cdiff, hdiff, tdiff], axis=-1), r


def similarity3_64(x, sp, hist, lbp, left, right, dense_w, dense_b, gamma):
    return _similarity3(x, sp, hist, lbp, left, right, dense_w, dense_b, gamma, np.float64)


def similarity3_32(x, sp, hist, lbp, left, right, dense_w, dense_b, gamma):
    return _similarity3(x, sp, hist, lbp, left, right, dense_w, dense_b, gamma, F)


def texture_bound(lbp, left, right, gamma, sp):
    """Per (image, pair) relative bound of the texture similarity, from the exact S_t."""
    S = s_t(lbp, left, right)
    assert S.max() < 2 ** 24
    return (4 * gamma * np.sqrt(S) / (sp * sp) + 3) * U


# ------------------------------------------------------------------------------------------------ cases
def dense3(seed=7):
    """dcnf_pair_ref.dense() with a third weight of the size of the other two."""
    w, b = P.dense(seed)
    return np.concatenate([w, [[F(0.625)]]]).astype(F), b


def measured():
    """Worst r error of the float32 form over the cases."""
    worst = 0.0
    w, b = dense3()
    for h, wd, sp in P.SHAPES:
        nsp = (h // sp) * (wd // sp)
        x = P.image(h, wd, sp, 3)
        hist, lbp = P.histogram(x, sp), lbp_histogram(x, sp)
        for gamma in P.GAMMAS:
            for length in (1, 100):
                left, right = P.pair_lists(nsp, length)
                _, r32 = similarity3_32(x, sp, hist, lbp, left, right, w, b, gamma)
                _, r64 = similarity3_64(x, sp, hist, lbp, left, right, w, b, gamma)
                worst = max(worst, P.r_errors(r32, r64).max())
    return float(worst)
