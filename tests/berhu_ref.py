"""Host references of the reverse Huber loss on linear depth (include/a3d_berhu.h: a3dh_berhu_loss_fwd / a3dh_berhu_loss_bwd_ex).

  loss64        numpy float64, the literal definition, with the closed-form gradient: what the kernels are held to
  literal_loss  torch float64 with the threshold detached, for autograd (tests/test_berhu_cpu.py pins loss64's gradient to it)
  loss32        numpy float32 in the header's order and partition, every operation rounded on its own (numpy has no FMA):
                chunks of ceil(npix / 8) rounded up to a multiple of 4, thread t of 256 adds pixels 1024 r + 4 t + {0..3} of
                its chunk to one accumulator in ascending order, the 64 accumulators of a wavefront as a tree with offsets 32,
                16, 8, 4, 2, 1, the four wavefronts ((w0 + w1) + w2) + w3, a sample's parts and then the samples in ascending
                order starting from 0.0f
  bound         8 x the worst error of loss32 against loss64 on the same inputs, computed on the CPU when a test asks; no figure
                comes from a kernel (the rule of tests/gradloss_ref.py)

Error measures: the loss |L - L64| / L64 (every term is >= 0, so nothing cancels); the gradient per sample
||g - g64||inf / ||g64||inf.  Both rho and the gradient are continuous at a = c (rho: (c^2 + c^2) / 2c = c; gradient: e / c =
sign e), so a pixel that float32 rounding puts on the other side of the threshold moves neither beyond rounding, and the bound
needs no term for it.  Only the COUNT of quadratic pixels, loss[3], is a step there: ambiguous() counts the pixels whose error
lies within rounding of the threshold, and loss[3] is held to the float64 count give or take those."""
import numpy as np

PARTS = 8            # A3D_SILOG_PARTS
F = np.float32


def counting(tgt, masked):
    return np.isfinite(tgt) if masked else np.ones(tgt.shape, bool)


def loss64(out, tgt, masked, fraction):
    """((loss, valid fraction, mean threshold, quadratic share), gradient [b, npix], c [b]) in float64."""
    o, t = np.asarray(out, np.float64), np.asarray(tgt, np.float64)
    b, npix = o.shape
    cnt = counting(t, masked)
    n = cnt.sum(axis=1)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        e = np.where(cnt, o - np.where(cnt, t, 0.0), 0.0)
        a = np.abs(e)
        poisoned = ~np.isfinite(a).all(axis=1)
        c = np.float64(fraction) * np.where(poisoned, np.nan, a.max(axis=1, initial=0.0))
        cc = c[:, None]
        linear = (a <= cc) | (cc == 0)
        rho = np.where(linear, a, (a * a + cc * cc) / np.where(cc == 0, 1.0, 2 * cc))
        rho = np.where(cnt, rho, 0.0)
        rn = np.where(n > 0, npix / np.maximum(n, 1), 0.0) if masked else np.ones(b)
        per = np.where(poisoned, np.nan, rn * rho.sum(axis=1))
        quad = cnt & ~linear
        s = (rn / b)[:, None]
        g = np.where(linear, np.sign(e) * s, e / np.where(cc == 0, 1.0, cc) * s)
        g = np.where(cnt & (e != 0), g, 0.0)
        g = np.where(poisoned[:, None], np.nan, g)
        l3 = np.nan if poisoned.any() else quad.sum() / n.sum() if n.sum() else 0.0
        losses = (per.sum() / b, n.sum() / (b * npix), c.sum() / b, l3)
    return losses, g, c


def literal_loss(out, tgt, masked, fraction):
    """loss[0] as a torch float64 scalar, the threshold detached: nothing is differentiated through the max."""
    import torch
    b, npix = out.shape
    cnt = torch.isfinite(tgt) if masked else torch.ones_like(tgt, dtype=torch.bool)
    total = out.new_zeros(())
    for i in range(b):
        if not cnt[i].any():
            continue
        e = out[i][cnt[i]] - tgt[i][cnt[i]]
        a = e.abs()
        c = (fraction * a.max()).detach()
        rho = a if c == 0 else torch.where(a <= c, a, (a * a + c * c) / (2 * c))
        total = total + (npix / int(cnt[i].sum()) if masked else 1.0) * rho.sum()
    return total / b


def _tree(v):
    """Lane 0 of v[l] += v[l + off], off = 32 .. 1, over the last axis of 64."""
    for off in (32, 16, 8, 4, 2, 1):
        v = v[..., :off] + v[..., off:2 * off]
    return v[..., 0]


def loss32(out, tgt, masked, fraction):
    """The same three values in float32, in the order and the partition include/a3d_berhu.h states."""
    o, t = np.asarray(out, F), np.asarray(tgt, F)
    b, npix = o.shape
    cnt = counting(t, masked)
    n = cnt.sum(axis=1)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        e = np.where(cnt, o - np.where(cnt, t, F(0)), F(0)).astype(F)
        a = np.abs(e)
        poisoned = ~np.isfinite(a).all(axis=1)
        c = (F(fraction) * np.where(poisoned, F(np.nan), a.max(axis=1, initial=F(0)))).astype(F)
        cc = c[:, None]
        linear = (a <= cc) | (cc == 0)
        quad_rho = ((a * a + cc * cc).astype(F) / np.where(cc == 0, F(1), F(2) * cc)).astype(F)
        rho = np.where(cnt, np.where(linear, a, quad_rho), F(0)).astype(F)
        # the partition: [b, parts, rounds, 256 threads, 4 pixels], what lies outside a chunk or the row adds +0.0
        chunk = ((npix + PARTS - 1) // PARTS + 3) & ~3
        rounds = (chunk + 1023) // 1024
        grid = np.zeros((b, PARTS, rounds * 1024), F)
        for part in range(PARTS):
            lo, hi = min(npix, part * chunk), min(npix, (part + 1) * chunk)
            grid[:, part, :hi - lo] = rho[:, lo:hi]
        grid = grid.reshape(b, PARTS, rounds, 256, 4)
        acc = np.zeros((b, PARTS, 256), F)
        for r in range(rounds):
            for u in range(4):
                acc = acc + grid[:, :, r, :, u]
        waves = _tree(acc.reshape(b, PARTS, 4, 64))
        parts = ((waves[..., 0] + waves[..., 1]) + waves[..., 2]) + waves[..., 3]
        S = np.zeros(b, F)
        for part in range(PARTS):
            S = S + parts[:, part]
        rn = (npix / np.maximum(n, 1).astype(np.float64)).astype(F) if masked else np.ones(b, F)
        per = np.where(n > 0, rn * S, F(0)).astype(F)
        l0, l2 = F(0), F(0)
        for i in range(b):
            l0, l2 = F(l0 + per[i]), F(l2 + c[i])
        quad = cnt & ~linear
        l3 = F(np.nan) if poisoned.any() else F(quad.sum() / n.sum()) if n.sum() else F(0)
        losses = (F(l0 / F(b)), F(n.sum() / (b * npix)) if masked else F(1), F(l2 / F(b)), l3)
        s = (F(F(1) / F(b)) * rn).astype(F)[:, None]
        g = np.where(linear, np.copysign(s, e), ((e / np.where(cc == 0, F(1), cc)).astype(F) * s).astype(F))
        g = np.where(cnt & (e != 0), g, F(0))
        g = np.where(poisoned[:, None], F(np.nan), g).astype(F)
    return losses, g, c


def rel(x, ref):
    x, ref = float(x), float(ref)
    return 0.0 if x == ref else abs(x - ref) / abs(ref) if ref else float('inf')


def grad_err(g, g64):
    """The worst per-sample ||g - g64||inf / ||g64||inf; a sample whose reference row is zero must be zero (then 0, else inf)."""
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    worst = 0.0
    for row, ref in zip(g, g64):
        top = np.abs(ref).max(initial=0.0)
        diff = np.abs(row - ref).max(initial=0.0)
        worst = max(worst, 0.0 if diff == 0 else diff / top if top else float('inf'))
    return worst


def ambiguous(out, tgt, masked, fraction):
    """The counting pixels whose |e| lies within 4 float32 roundings of the sample's threshold: only they may fall on either
    side of it in float32."""
    o, t = np.asarray(out, np.float64), np.asarray(tgt, np.float64)
    cnt = counting(t, masked)
    a = np.abs(np.where(cnt, o - np.where(cnt, t, 0.0), 0.0))
    c = fraction * a.max(axis=1, initial=0.0)[:, None]
    return int((cnt & (np.abs(a - c) <= 4 * 2.0 ** -24 * c)).sum())


def bound(out, tgt, masked, fraction):
    """(float64 losses, float64 gradient, loss bound, gradient bound): the bounds are 8 x what loss32 shows against loss64 on
    these inputs, the loss bound the worse of loss[0]'s and loss[2]'s."""
    l64, g64, _ = loss64(out, tgt, masked, fraction)
    l32, g32, _ = loss32(out, tgt, masked, fraction)
    return l64, g64, 8 * max(rel(l32[0], l64[0]), rel(l32[2], l64[2])), 8 * grad_err(g32, g64)


def case(b, npix, seed, masked):
    """(out, tgt) float32 [b, npix]: targets uniform in (0.05, 1); outputs the target plus a normal error of 0.3, so that a
    good share lie at or below zero (where the log loss has no gradient) and the errors spread around every threshold.
    masked: holes (NaN, a few inf) as a run and a sprinkle, their outputs untouched, and with b >= 3 the middle sample
    without a finite target at all."""
    rng = np.random.default_rng(seed)
    t = (rng.random((b, npix), dtype=F) * F(0.95) + F(0.05)).astype(F)
    o = (t + rng.standard_normal((b, npix)).astype(F) * F(0.3)).astype(F)
    if masked:
        hole = rng.random((b, npix)) < 0.2
        hole[:, npix // 3:npix // 3 + npix // 5] = True
        if npix > 1:
            hole[:, 0] = False
        else:
            hole[:] = False
        if b >= 3:
            hole[b // 2] = True
        t[hole] = np.nan
        t[hole & (rng.random((b, npix)) < 0.1)] = np.inf
    return o, t


def integer_case(b, npix, seed=0):
    """Integer-valued o and t with |e| in {0, 1, 2, 3, 4}, every sample holding a 4, and exactly every other pixel a hole:
    with fraction 0.5 the threshold is 2, rho lies in {0, 1, 2, 3.25, 5}, r_n = 2, and at b in {1, 2, 4} every float32
    operation of the header is exact in any order (exact_conditions asserts it)."""
    assert npix % 2 == 0 and npix >= 4
    rng = np.random.default_rng(seed)
    t = rng.integers(1, 9, (b, npix)).astype(F)
    e = rng.integers(-4, 5, (b, npix)).astype(F)
    e[:, 0], e[:, npix - 2] = 4, -4                     # even columns count: the maximum at both ends of the counting pixels
    o = (t + e).astype(F)
    t[:, 1::2] = np.nan
    e[:, 1::2] = 8                                      # a larger error on every hole: it must not set the threshold
    o[:, 1::2] = 8
    return o, t


def exact_conditions(o, t, fraction=0.5):
    """What makes integer_case exact: whole-number errors up to 4 on the counting pixels, c = 2, r_n = 2, b a power of two,
    and sums of multiples of 1/4 far below 2^24 / 4."""
    b, npix = o.shape
    cnt = np.isfinite(t)
    e = (o.astype(np.float64) - np.where(cnt, t, 0).astype(np.float64))[cnt]
    assert (e == np.round(e)).all() and np.abs(e).max() == 4 and fraction * 4 == 2
    assert (np.abs((o.astype(np.float64) - np.where(cnt, t, 0))).reshape(b, -1)[:, ::2].max(axis=1) == 4).all()
    assert (cnt.sum(axis=1) * 2 == npix).all() and b & (b - 1) == 0
    assert 5 * npix * b * 2 < 2 ** 22
