"""Host reference (numpy only) of the scale-invariant log loss with the gradient-matching term of Eigen & Fergus 2015
(include/a3d_gradloss.h: a3dg_silog_grad_loss_fwd / a3dg_silog_grad_loss_bwd_ex), in the caller's dtype: called on float64
arrays it is the reference the kernels are held to, called on float32 arrays it is the float32 restatement whose error against
the float64 run sets the kernels' tolerance (numpy's pairwise sums, not the kernels' order).  tests/test_gradloss_cpu.py pins it
to torch autograd of the literal loss and, at weight 0, to tests/valid_ref.py."""
import numpy as np

EPS = 1e-8
SILOG_C = float(np.float32(0.5 / (74 * 55)))      # the reference's folded constant (src/models.py:269), whatever npix is


def _masked_log(v):
    with np.errstate(invalid='ignore', divide='ignore'):
        l = np.log(v + v.dtype.type(EPS))
    nan = np.isnan(l)
    return np.where(nan, v.dtype.type(0), l), nan


def _terms(out, tgt, h, w, masked):
    b = out.shape[0]
    o, t = out.reshape(b, h, w), tgt.reshape(b, h, w)
    dt = o.dtype.type
    valid = np.isfinite(t) if masked else np.ones(t.shape, bool)
    lo, nan_o = _masked_log(o)
    lt, _ = _masked_log(np.where(valid, t, dt(1)))
    d = np.where(valid, lo - lt, dt(0))
    n = valid.reshape(b, -1).sum(axis=1)
    vh, vv = valid[:, :, 1:] & valid[:, :, :-1], valid[:, 1:] & valid[:, :-1]        # the pairs that count
    with np.errstate(invalid='ignore', over='ignore'):
        dh = np.where(vh, d[:, :, 1:] - d[:, :, :-1], dt(0))
        dv = np.where(vv, d[:, 1:] - d[:, :-1], dt(0))
    m = vh.reshape(b, -1).sum(axis=1) + vv.reshape(b, -1).sum(axis=1)
    pairs = h * (w - 1) + (h - 1) * w
    if masked:
        safe = np.maximum(n, 1).astype(np.float64)
        cn, rn = (0.5 / safe).astype(o.dtype), (h * w / safe).astype(o.dtype)
        rm = np.where(m > 0, pairs / np.maximum(m, 1).astype(np.float64), 0.0).astype(o.dtype)
    else:
        cn, rn, rm = np.full(b, dt(SILOG_C)), np.ones(b, o.dtype), np.ones(b, o.dtype)
    return o, d, valid, nan_o, n, m, dh, dv, cn, rn, rm


def grad_loss_fwd(out, tgt, h, w, masked, grad_weight):
    """(total, valid fraction, silog part, gradient part), each the mean over the batch; out / tgt [b, h w] or [b, h, w]."""
    o, d, valid, _, n, m, dh, dv, cn, rn, rm = _terms(out, tgt, h, w, masked)
    b = o.shape[0]
    dt = o.dtype.type
    flat = d.reshape(b, -1)
    with np.errstate(invalid='ignore', over='ignore'):
        per = rn * ((flat * flat).sum(axis=1) - cn * np.square(flat.sum(axis=1)))
        per = np.where(n > 0, per, dt(0))
        sg = (dh * dh).reshape(b, -1).sum(axis=1) + (dv * dv).reshape(b, -1).sum(axis=1)
        gpart = np.where(m > 0, rm * sg, dt(0))
        silog, grad = per.mean(dtype=o.dtype), gpart.mean(dtype=o.dtype)
        total = silog if grad_weight == 0 else silog + dt(grad_weight) * grad
    return total, n.sum() / (b * h * w), silog, grad


def grad_loss_bwd(out, tgt, h, w, masked, grad_weight):
    """d total / d out: 0 where log(o + 1e-8) is NaN and where the pixel does not count."""
    o, d, valid, nan_o, n, m, dh, dv, cn, rn, rm = _terms(out, tgt, h, w, masked)
    b = o.shape[0]
    dt = o.dtype.type
    sd = d.reshape(b, -1).sum(axis=1)[:, None, None]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        g = (dt(2) * d - (dt(2) * cn[:, None, None]) * sd) * dt(1.0 / b) * rn[:, None, None]
        if grad_weight != 0:
            lap = np.zeros_like(d)              # sum over the counting pairs of a pixel of (d_i - d_j)
            lap[:, :, 1:] += dh
            lap[:, :, :-1] -= dh
            lap[:, 1:] += dv
            lap[:, :-1] -= dv
            g = g + dt(2) * (dt(grad_weight) * rm[:, None, None]) * lap * dt(1.0 / b)
        g = g / (o + dt(EPS))
    g = np.where(valid & ~nan_o, g, dt(0))
    return g.reshape(out.shape).astype(out.dtype, copy=False)


def loss_case(b, h, w, seed, invalid=None):
    """(out, tgt) float32 [b, h w]: o and t uniform in (0.05, 1) and independent, so that neighbouring d differ by O(1); 4 %
    of the outputs negated (o < -1e-8: log is NaN, the NaN -> 0 rule is live; no o + 1e-8 is 0).  invalid=None: holes (NaN,
    a few of them inf) as two blobs per sample, the second touching the last row and the last column, plus a sprinkle of
    single pixels, and sample b - 1 without a finite target at all (a 1 x 1 grid: only that).  invalid=0: no hole."""
    rng = np.random.default_rng(seed)
    o = (rng.random((b, h, w), dtype=np.float32) * np.float32(0.95) + np.float32(0.05)).astype(np.float32)
    t = (rng.random((b, h, w), dtype=np.float32) * np.float32(0.95) + np.float32(0.05)).astype(np.float32)
    neg = rng.random((b, h, w)) < 0.04
    if h * w > 1:
        neg[0, 0, 0], neg[0, -1, -1] = False, True
    o[neg] = -o[neg]
    if invalid is None:
        hole = np.zeros((b, h, w), bool)
        if h * w > 1:
            r0, c0 = h // 4, w // 4
            hole[:, r0:r0 + max(1, h // 3), c0:c0 + max(1, w // 3)] = True
            hole[:, h - max(1, h // 5):, w - max(1, w // 5):] = True
            hole |= rng.random((b, h, w)) < 0.03
            hole[:, 0, 0] = False
        hole[-1] = True
        t[hole] = np.nan
        t[hole & (rng.random((b, h, w)) < 0.1)] = np.inf
    else:
        assert invalid == 0
    return o.reshape(b, h * w), t.reshape(b, h * w)


def constant_case(b, h, w, masked):
    """Every sample's d is one constant: o and t constant per sample (so sg is exactly 0), with loss_case's holes if masked."""
    o = np.repeat(np.linspace(0.2, 0.9, b, dtype=np.float32)[:, None], h * w, axis=1)
    t = np.repeat(np.linspace(0.8, 0.1, b, dtype=np.float32)[:, None], h * w, axis=1)
    if masked:
        t[~np.isfinite(loss_case(b, h, w, 0)[1])] = np.nan
    return np.ascontiguousarray(o), np.ascontiguousarray(t)


def rel(x, ref):
    x, ref = float(x), float(ref)
    return 0.0 if x == ref else abs(x - ref) / abs(ref) if ref else float('inf')


def rel_l2(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(x - ref) / max(np.linalg.norm(ref), 1e-300))


WEIGHTS = (0.5, 1.0)


def tolerances(o, t, h, w, masked):
    """({weight: (float64 forward, float64 backward)}, loss bound, gradient bound) for the weights the GPU tests run on these
    inputs.  The bounds are 8 x the error the float32 restatement shows against float64 on these same inputs: the worst
    relative error over total, silog part and gradient part at either weight, and the worse rel-L2 error of the gradient (one
    draw of a rounding error can come out near zero; the worst of the figures the same inputs give does not)."""
    o64, t64 = o.astype(np.float64), t.astype(np.float64)
    refs, e_loss, e_grad = {}, 0.0, 0.0
    for weight in WEIGHTS:
        f64, g64 = grad_loss_fwd(o64, t64, h, w, masked, weight), grad_loss_bwd(o64, t64, h, w, masked, weight)
        f32, g32 = grad_loss_fwd(o, t, h, w, masked, weight), grad_loss_bwd(o, t, h, w, masked, weight)
        e_loss = max([e_loss] + [rel(f32[k], f64[k]) for k in (0, 2, 3)])
        e_grad = max(e_grad, rel_l2(g32, g64))
        refs[weight] = (f64, g64)
    return refs, 8 * e_loss, 8 * e_grad
