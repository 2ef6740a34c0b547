"""References of the DCNF pairwise kernels (superpixel_mean / superpixel_hist / pair_similarity, src/models.py:91-127) for
any image size (h, w), superpixel edge sp, channel count c, pair lists and gamma; float64 forms and float32 forms in the
kernels' order of operations (tests/test_crf_loss_cpu.py, tests/test_gpu_dcnf_pairwise.py, tests/test_gpu_dcnf.py).

blocks(x, sp)            [n, h, w, c] -> [n, P, sp * sp, c], superpixels row-major, pixels row-major inside one
means64 / means32        block means [n, P, c]
histogram(x, sp)         the oracle's separately rounded float32 operations in the oracle's order (oracle.dcnf.
                         color_histogram, oracle.tf13_ops.histogram_fixed_width): (r * 2^24 + g * 2^16) + b * 2^8, / 2^24,
                         floor(256 * .), clipped to [0, 255]; integer counts [n, P, 256] (float32, exact)
similarity64 / 32        (sims [n, Q, 2], r [n, Q]) from an image, its histogram, pair lists, the 2 -> 1 dense layer, gamma

The float32 forms sum as the kernels do: thread t of 256 adds pixels t, t + 256, ... in order, the 64 lanes of each of
the four wavefronts by the butterfly of crf_loss_ref._wave_sum, then ((w0 + w1) + w2) + w3.

Bounds.  Over SHAPES x CHANNELS for the means and SHAPES x GAMMAS x pair lists of length 1 and 100 for the similarities
(the cases of tests/test_gpu_dcnf_pairwise.py; measured() below) the float32 forms lie from float64 by at most
                                                         measured     bound = 8 x    kernel on an MI355X reached
  block means                                            1.41e-07     1.2e-06        1.41e-07
  colour similarity                                      3.05e-06     2.5e-05        2.99e-06
  r                                                      2.06e-07     1.7e-06        2.06e-07
and the kernels are held to 8 x that, the margin of tests/test_gpu_crf_map.py.  The errors are per element and relative
for the means (against max(|mean64|, mean64 of |x|): a mean that cancels is held to the size of what was summed) and for
the colour similarity, and per image ||.||inf-relative for r; a result below the float32 normal range may be flushed.

The histogram similarity needs no measurement.  The counts are integers, their differences and S = sum d^2 < 2^24 are
exact in float32 in any order, and what remains is expf(-gamma * sqrtf(S)): sqrtf within 1 ulp (2u, u = 2^-24), the
product rounded once (u), so the argument t = -gamma sqrt(S) carries a relative error of at most 3u, which expf turns
into |t| 3u of its result; expf's own error is at most 1 ulp (2u).  hist_bound(t) = (3 |t| + 3) u, the last u for the
second-order terms.  The kernel on an MI355X reached 0.294 of it at the worst.
"""
import numpy as np

from crf_loss_ref import F, FLT_MIN, U, _wave_sum

# 8 x the measured worst, rounded up to two digits
MEAN_BOUND, COLOR_BOUND, R_BOUND = 1.2e-06, 2.5e-05, 1.7e-06


def blocks(x, sp):
    n, h, w, c = x.shape
    v = x.reshape(n, h // sp, sp, w // sp, sp, c).transpose(0, 1, 3, 2, 4, 5)
    return v.reshape(n, (h // sp) * (w // sp), sp * sp, c)


def _block_sum32(v):
    """block_sum_256 of crf.hip over the last axis of float32 v [..., m] after each thread's own serial sum."""
    lead, m = v.shape[:-1], v.shape[-1]
    k = -(-m // 256)
    pad = np.zeros(lead + (k * 256,), F)
    pad[..., :m] = v
    pad = pad.reshape(-1, k, 256)
    t = np.zeros((pad.shape[0], 256), F)
    for i in range(k):
        t = t + pad[:, i]
    wsum = [_wave_sum(t[:, 64 * i:64 * i + 64]) for i in range(4)]
    return (((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]).reshape(lead)


def means64(x, sp):
    return blocks(np.asarray(x, np.float64), sp).mean(axis=2)


def means32(x, sp):
    b = blocks(np.ascontiguousarray(x, F), sp)                   # [n, P, m, c]
    return _block_sum32(np.ascontiguousarray(b.transpose(0, 1, 3, 2))) / F(sp * sp)


def histogram(x, sp):
    b = blocks(np.ascontiguousarray(x, F), sp)
    assert b.shape[-1] == 3
    with np.errstate(all='ignore'):
        v = (b[..., 0] * F(16777216.) + b[..., 1] * F(65536.)) + b[..., 2] * F(256.)
        scaled = (v - F(0)) / (F(16777216.) - F(0))
        idx = np.clip(np.floor(F(256) * scaled).astype(np.int64), 0, 255)
    n, P, m = idx.shape
    flat = (np.arange(n * P)[:, None] * 256 + idx.reshape(n * P, m)).ravel()
    return np.bincount(flat, minlength=n * P * 256).reshape(n, P, 256).astype(F)


def _similarity(x, sp, hist, left, right, dense_w, dense_b, gamma, dt):
    left, right = np.asarray(left, np.int64), np.asarray(right, np.int64)
    x = np.ascontiguousarray(x, dt)
    dw, db = np.asarray(dense_w, dt).ravel(), np.asarray(dense_b, dt).ravel()
    b = blocks(x, sp)
    gray = ((b[..., 0] + b[..., 1]) + b[..., 2]) / dt(3)          # [n, P, m]
    d = gray[:, left] - gray[:, right]
    dh = np.asarray(hist, dt)[:, left] - np.asarray(hist, dt)[:, right]
    with np.errstate(under='ignore'):
        if dt is F:
            sc, sh = _block_sum32(d * d), _block_sum32(dh * dh)
        else:
            sc, sh = (d * d).sum(axis=2), (dh * dh).sum(axis=2)
        cdiff, hdiff = np.exp(-dt(gamma) * np.sqrt(sc)), np.exp(-dt(gamma) * np.sqrt(sh))
        r = (cdiff * dw[0] + hdiff * dw[1]) + db[0]
    return np.stack([cdiff, hdiff], axis=-1), r, sh


def similarity64(x, sp, hist, left, right, dense_w, dense_b, gamma):
    return _similarity(x, sp, hist, left, right, dense_w, dense_b, gamma, np.float64)[:2]


def similarity32(x, sp, hist, left, right, dense_w, dense_b, gamma):
    return _similarity(x, sp, hist, left, right, dense_w, dense_b, gamma, F)[:2]


def hist_bound(x_hist, left, right, gamma):
    """Per (image, pair) relative bound of the histogram similarity, from the exact S."""
    h = np.asarray(x_hist, np.float64)
    d = h[:, np.asarray(left, np.int64)] - h[:, np.asarray(right, np.int64)]
    S = (d * d).sum(axis=2)
    assert S.max() < 2 ** 24
    return (3 * gamma * np.sqrt(S) + 3) * U


# ------------------------------------------------------------------------------------------------ errors
def mean_errors(got, x, sp):
    want = means64(x, sp)
    scale = np.maximum(np.abs(want), blocks(np.abs(np.asarray(x, np.float64)), sp).mean(axis=2))
    return np.abs(np.asarray(got, np.float64) - want) / np.maximum(scale, FLT_MIN)


def rel_errors(got, want):
    """Per element, relative; a result below the float32 normal range may have been flushed to 0."""
    want = np.asarray(want, np.float64)
    return np.maximum(np.abs(np.asarray(got, np.float64) - want) - FLT_MIN, 0) / np.maximum(np.abs(want), FLT_MIN)


def r_errors(got, want):
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want).max(axis=1) / np.abs(want).max(axis=1)


# ------------------------------------------------------------------------------------------------ cases
SHAPES = [(240, 320, 40), (40, 40, 40), (16, 48, 16), (24, 8, 8), (16, 16, 16), (8, 8, 8), (32, 48, 16), (48, 16, 8)]
GAMMAS = [0.25, 1.0, 4.0]
CHANNELS = [1, 3, 4]


def image(h, w, sp, n, c=3, seed=0):
    """n images: the first tiles one random superpixel over the grid and changes a few pixels (both similarities well
    inside (0, 1)), the second is smooth (colour similarity in range), the third white noise."""
    rng = np.random.default_rng(1000 * h + 10 * w + sp + 7 * c + seed)
    img = np.empty((n, h, w, c), F)
    for i in range(n):
        kind = i % 3
        if kind == 0:
            img[i] = np.tile(rng.random((sp, sp, c)).astype(F), (h // sp, w // sp, 1))
            for _ in range(max(4, h * w // 1280)):
                img[i, rng.integers(h), rng.integers(w)] = rng.random(c).astype(F)
        elif kind == 1:
            base = rng.random((h // sp, w // sp, c)).astype(F)
            img[i] = np.kron(base, np.ones((sp, sp, 1), F)) * F(0.02) + F(0.4)
            img[i] += (rng.random(img[i].shape).astype(F) - F(0.5)) * F(0.004)
        else:
            img[i] = rng.random((h, w, c)).astype(F)
    return img


def pair_lists(nsp, length, seed=0):
    """Random pairs with repeats and non-neighbours; the first has left == right when there is room."""
    rng = np.random.default_rng(nsp + 100 * length + seed)
    left, right = rng.integers(0, nsp, length), rng.integers(0, nsp, length)
    if length > 1:
        right[0] = left[0]
    return left.astype(np.int32), right.astype(np.int32)


def dense(seed=7):
    from oracle import dcnf as OD
    p = OD.pairwise_init(seed)
    w, b = p[OD.PAIR_PREFIX + 'kernel'].copy(), p[OD.PAIR_PREFIX + 'bias'].copy()
    b[0] = F(0.03125)                                            # a bias that is not 0, so that it is seen
    return w, b


def measured():
    """(worst mean error, worst colour-similarity error, worst r error) of the float32 forms over the cases."""
    worst = np.zeros(3)
    w, b = dense()
    for h, wd, sp in SHAPES:
        nsp = (h // sp) * (wd // sp)
        for c in CHANNELS:
            x = image(h, wd, sp, 3, c)
            worst[0] = max(worst[0], mean_errors(means32(x, sp), x, sp).max())
        x = image(h, wd, sp, 3)
        hist = histogram(x, sp)
        for gamma in GAMMAS:
            for length in (1, 100):
                left, right = pair_lists(nsp, length)
                s32, r32 = similarity32(x, sp, hist, left, right, w, b, gamma)
                s64, r64 = similarity64(x, sp, hist, left, right, w, b, gamma)
                worst[1] = max(worst[1], rel_errors(s32[..., 0], s64[..., 0]).max())
                worst[2] = max(worst[2], r_errors(r32, r64).max())
    return tuple(float(v) for v in worst)
