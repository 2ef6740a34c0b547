"""Host reference of include/a3d_align.h (a helper, not a test): the pixel set, the lower medians by sorting integer keys,
the least-squares coefficients EXACTLY (fractions.Fraction on the float32 values, rounded to float32 once), the conditioning
the one-ulp bound of tests/test_gpu_align.py rests on, and the aligned metric rows."""
from fractions import Fraction

import numpy as np

from oracle import tf13_ops as T
from test_eval_cpu import ref_rows

MODES = ('median', 'scale', 'affine')
EXACT = [0, 7, 8, 9, 10]                    # counts: n, the three deltas, non-finite
CONT = [1, 2, 3, 4, 5, 6]


def sampled(pred, th, tw):
    """pred [n, ph, pw] at the pixels of a th x tw target: the legacy resize, which the kernels reproduce bit for bit
    (tests/test_gpu_eval.py), or pred itself when the grids agree."""
    pred = np.asarray(pred, np.float32)
    if pred.shape[1:] == (th, tw):
        return pred
    return T.resize_bilinear_tf1(pred[..., None], th, tw)[..., 0]


def fit_mask(p, t, min_depth=0., max_depth=np.inf):
    """The pixels an image is fitted on, validity as test_eval_cpu.ref_rows: p, t on the same grid."""
    with np.errstate(invalid='ignore'):
        return np.isfinite(t) & (t > np.float32(min_depth)) & (t <= np.float32(max_depth)) & np.isfinite(p)


def order_key(x):
    """The total order of the selection: float bits, all flipped for a negative, the sign bit flipped otherwise."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, u ^ 0xFFFFFFFF, u ^ 0x80000000)


def key_value(k):
    k = np.int64(k)
    u = (k ^ 0x80000000) if (k & 0x80000000) else (k ^ 0xFFFFFFFF)
    return np.array([u], np.uint32).view(np.float32)[0]


def lower_median(x):
    """The element of 0-based rank (m - 1) // 2 in the order of order_key: no averaging."""
    k = np.sort(order_key(np.asarray(x, np.float32).ravel()))
    return key_value(k[(len(k) - 1) // 2])


def fl32(x):
    """A Fraction correctly rounded to float32 (ties to even); inf past the largest float32."""
    if x == 0:
        return np.float32(0)
    big = Fraction(float(np.finfo(np.float32).max))
    half_ulp_big = Fraction(2) ** 103
    if abs(x) >= big + half_ulp_big:
        return np.float32(np.inf if x > 0 else -np.inf)
    with np.errstate(over='ignore'):
        c = np.float32(float(x))                       # within one float32 step of the answer
    if not np.isfinite(c):
        c = np.float32(np.finfo(np.float32).max if x > 0 else -np.finfo(np.float32).max)
    with np.errstate(over='ignore'):
        cands = [c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))]
    cands = [v for v in cands if np.isfinite(v)]

    def even(v):
        return (int(np.array([v], np.float32).view(np.uint32)[0]) & 1) == 0
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - x), not even(v)))


def ref_align(pred, target, mode, min_depth=0., max_depth=np.inf):
    """pred [n, ph, pw], target [n, th, tw] float32 (a uint8 record expanded by data.expand_u8).  Returns a dict: coef
    float32 [n, 2], count, status int32 [n], kappa [n] = S_pp / (S_pp - S_p^2 / m) (1 outside 'affine', inf when the
    denominator is 0) and cond [n] = sum |terms| / |numerator| of s (1 for 'median')."""
    target = np.asarray(target, np.float32)
    n, th, tw = target.shape
    ps = sampled(pred, th, tw)
    coef = np.tile(np.array([1, 0], np.float32), (n, 1))
    count = np.zeros(n, np.int32)
    status = np.ones(n, np.int32)
    kappa, cond = np.ones(n), np.ones(n)
    for i in range(n):
        ok = fit_mask(ps[i], target[i], min_depth, max_depth)
        p, t = ps[i][ok], target[i][ok]
        m = count[i] = len(p)
        if mode == 'median':
            if m < 1:
                continue
            mt, mp = lower_median(t), lower_median(p)
            with np.errstate(divide='ignore', over='ignore', invalid='ignore', under='ignore'):
                s = np.float32(mt) / np.float32(mp)
            if mp > 0 and np.isfinite(s) and s > 0:
                coef[i], status[i] = (s, 0), 0
            continue
        fp = [Fraction(float(v)) for v in p]
        ft = [Fraction(float(v)) for v in t]
        sp, st = sum(fp, Fraction(0)), sum(ft, Fraction(0))
        spp = sum((a * a for a in fp), Fraction(0))
        spt = sum((a * b for a, b in zip(fp, ft)), Fraction(0))
        if mode == 'scale':
            if m < 1 or spp <= 0:
                continue
            s = fl32(spt / spp)
            cond[i] = float(sum(abs(a * b) for a, b in zip(fp, ft)) / abs(spt)) if spt != 0 else np.inf
            if np.isfinite(s) and s > 0:
                coef[i], status[i] = (s, 0), 0
            continue
        if m < 2:
            continue
        den = spp - sp * sp / m
        if den <= 0:
            kappa[i] = np.inf
            continue
        kappa[i] = float(spp / den)
        num = spt - sp * st / m
        cond[i] = float((sum(abs(a * b) for a, b in zip(fp, ft)) + abs(sp * st / m)) / abs(num)) if num != 0 else np.inf
        s = num / den
        b = (st - s * sp) / m
        s32, b32 = fl32(s), fl32(b)
        if np.isfinite(s32) and np.isfinite(b32):
            coef[i], status[i] = (s32, b32), 0
    return dict(coef=coef, count=count, status=status, kappa=kappa, cond=cond)


def apply(x, coef):
    """fl32(fl32(s x) + b) per image: two float32 roundings."""
    x = np.asarray(x, np.float32)
    c = np.asarray(coef, np.float32).reshape(len(x), 2, *([1] * (x.ndim - 1)))
    with np.errstate(invalid='ignore', over='ignore'):
        return (c[:, 0] * x).astype(np.float32) + c[:, 1]


def aligned_rows(pred, target, coef, magnitude=False, **kw):
    """The rows of a3da_depth_metrics_aligned: ref_rows of the sampled prediction after apply()."""
    target = np.asarray(target, np.float32)
    return ref_rows(apply(sampled(pred, *target.shape[1:]), coef), target, magnitude=magnitude, **kw)


def check_rows(got, want, scale):
    """The rule tests/test_gpu_eval.py holds a3d_depth_metrics to: counts exact, continuous columns within 1e-5 of the
    column's sum of magnitudes."""
    np.testing.assert_array_equal(got[:, EXACT], want[:, EXACT])
    err = np.abs(got[:, CONT] - want[:, CONT])
    assert (err <= 1e-5 * scale[:, CONT] + 1e-30).all(), (err / np.maximum(scale[:, CONT], 1e-30)).max()


def ulps(a, b):
    """Distance in float32 steps between same-shaped finite arrays."""
    return np.abs(order_key(a) - order_key(b))
