"""Host references (numpy only) of the training path for depth maps with holes: the validity-aware resize / warp of
include/a3d_valid.h (a3dx_resize_bilinear_tf1_valid, a3dx_warp_bilinear_pair_valid) on top of tests/augment_ref.py, and the masked
scale-invariant loss (a3dx_silog_masked_loss_fwd / _bwd_ex) in the caller's dtype.  tests/test_valid_cpu.py pins them to
augment_ref.warp, to the oracle's loss and to torch autograd; the GPU tests hold the kernels to them."""
import numpy as np

import augment_ref as R

EPS = 1e-8


def resize_valid(x, table, oh, ow, min_depth, max_depth):
    """x [n, h, w, c] float32 or uint8, a depth map (tensor 1 of the launch: the table's depth gain) -> [n, oh, ow, c]
    float32.  augment_ref.identity(n) as the table: the plain resize.  An element is augment_ref.warp's where every
    counting tap (tl always, tr iff lx > 0, bl iff ly > 0, br iff both) is finite with min_depth < t <= max_depth and all
    four taps are finite; NaN elsewhere."""
    n, h, w, c = x.shape
    y = R.warp(x, table, oh, ow, second=True)
    xf = R.as_float(x)
    fx, fy = R.coords(table, h, w, oh, ow)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    px = ((fx - x0.astype(np.float32)) > 0)[..., None]
    py = ((fy - y0.astype(np.float32)) > 0)[..., None]
    b = np.arange(n)[:, None, None]
    lo, hi = np.float32(min_depth), np.float32(max_depth)

    def ok(t, counts):
        with np.errstate(invalid='ignore'):
            valid = np.isfinite(t) & (t > lo) & (t <= hi)
        return np.where(counts, valid, np.isfinite(t))
    good = (ok(xf[b, y0, x0], True) & ok(xf[b, y0, x1], px) & ok(xf[b, y1, x0], py) & ok(xf[b, y1, x1], px & py))
    return np.where(good, y, np.float32(np.nan)).astype(np.float32)


def _masked_log(v):
    with np.errstate(invalid='ignore', divide='ignore'):
        l = np.log(v + v.dtype.type(EPS))
    nan = np.isnan(l)
    return np.where(nan, v.dtype.type(0), l), nan


def _sums(out, tgt):
    b = out.shape[0]
    o, t = out.reshape(b, -1), tgt.reshape(b, -1)
    dt = o.dtype.type
    valid = np.isfinite(t)
    lo, nan_o = _masked_log(o)
    lt, _ = _masked_log(np.where(valid, t, dt(1)))
    d = np.where(valid, lo - lt, dt(0))
    n = valid.sum(axis=1)
    npix = o.shape[1]
    safe = np.maximum(n, 1).astype(np.float64)
    cn = (0.5 / safe).astype(o.dtype)
    rn = (npix / safe).astype(o.dtype)
    return o, d, valid, nan_o, n, cn, rn


def masked_silog_fwd(out, tgt):
    """(loss, valid fraction).  Per sample r_n (s2 - c_n s1^2) over its finite targets, 0 for a sample without one; the
    mean over the batch."""
    o, d, valid, _, n, cn, rn = _sums(out, tgt)
    with np.errstate(invalid='ignore', over='ignore'):
        per = rn * ((d * d).sum(axis=1) - cn * np.square(d.sum(axis=1)))
    per = np.where(n > 0, per, o.dtype.type(0))
    return per.mean(dtype=o.dtype), n.sum() / (o.shape[0] * o.shape[1])


def masked_silog_bwd(out, tgt):
    """d loss / d out: 0 at holes, at outputs whose log is NaN and in a sample without a valid pixel."""
    o, d, valid, nan_o, n, cn, rn = _sums(out, tgt)
    dt = o.dtype.type
    sd = d.sum(axis=1, keepdims=True)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        g = (dt(2) * d - (dt(2) * cn[:, None]) * sd) * dt(1.0 / o.shape[0]) * rn[:, None]
        g = g / (o + dt(EPS))
    g = np.where(valid & ~nan_o, g, dt(0))
    return g.reshape(out.shape).astype(out.dtype, copy=False)


def loss_case(b, npix, seed, invalid=None):
    """(out, tgt) float32 [b, npix] for the loss tests: outputs with negative values (the NaN -> 0 rule is live), targets
    in (0.05, 10] with a share `invalid` of NaN holes (default: drawn per sample from 30..90 %), a few of them infinite,
    sample b - 1 without a single valid pixel, and one valid target of exactly 0."""
    rng = np.random.default_rng(seed)
    o = (rng.random((b, npix), dtype=np.float32) * np.float32(3) - np.float32(0.4)).astype(np.float32)
    t = (rng.random((b, npix), dtype=np.float32) * np.float32(9.95) + np.float32(0.05)).astype(np.float32)
    share = rng.uniform(0.3, 0.9, (b, 1)) if invalid is None else np.full((b, 1), invalid)
    hole = rng.random((b, npix)) < share
    if invalid is None:
        hole[:, 0] = False                       # every sample but the last keeps a valid pixel ...
        hole[-1] = True                          # ... the last has none
    t[hole] = np.nan
    t[hole & (rng.random((b, npix)) < 0.05)] = np.inf
    if invalid is None and b > 1:
        t[0, 0] = 0                              # valid, and takes log(1e-8)
        o[0, 0] = np.float32(0.5)
    return o, t


def rel_l2(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(x - ref) / max(np.linalg.norm(ref), 1e-300))
