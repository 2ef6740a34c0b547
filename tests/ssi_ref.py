"""Host references of the least-squares scale-and-shift-invariant loss on linear depth (include/a3d_ssi.h: a3di_ssi_loss_fwd /
a3di_ssi_loss_bwd_ex).

  loss64        numpy float64, the literal definition, with the closed-form gradient s r k (s and t unrounded): what the kernels
                are held to
  literal_loss  torch float64 with the fit by an explicit least-squares solve that autograd differentiates THROUGH
                (tests/test_ssi_cpu.py pins loss64's gradient to it: the envelope-theorem claim of the header)
  loss32        the header's arithmetic, order and partition: the four float64 sums per thread in ascending pixel order (chunks
                of ceil(npix / 8) rounded up to a multiple of 4, thread t of 256 takes pixels 1024 r + 4 t + {0..3} of its
                chunk), the 64 accumulators of a wavefront as a tree with offsets 32, 16, 8, 4, 2, 1, the four wavefronts
                ((w0 + w1) + w2) + w3, a sample's parts in ascending order from 0; the solve in float64, operation by operation;
                then the float32 residual walk in the same partition, every operation rounded on its own (numpy has no FMA)
  bound         8 x the worst error of loss32 against loss64 on the same inputs, computed on the CPU when a test asks; no figure
                comes from a kernel (the rule of tests/berhu_ref.py)

Error measures: the loss |L - L64| / L64 (every term is >= 0, so nothing cancels); the mean scale and the mean shift against
the mean MAGNITUDE of the samples' float64 values (a mean shift may cancel to nothing); the gradient per sample
||g - g64||inf / ||g64||inf.  Every quantity is continuous in the inputs away from the degenerate floor, and case() keeps
den / S_oo near 0.3, so the bound needs no term for a sample that rounding puts on the other side of the floor."""
import numpy as np

PARTS = 8            # A3D_SILOG_PARTS
F = np.float32
FITTED, DEGENERATE, POISONED = 0, 1, 2
FLOOR = 2.0 ** -30


def counting(tgt, masked):
    return np.isfinite(tgt) if masked else np.ones(tgt.shape, bool)


def poisoned_rows(o, t, cnt, masked):
    bad = cnt & ~np.isfinite(o)
    if not masked:
        bad = bad | ~np.isfinite(t)
    return bad.any(axis=1)


def solve(s_o, s_d, s_oo, s_od, n):
    """The header's fit from the four sums of one sample, every operation a float64 operation of its own:
    (s64, t64, fitted) before the float32 tests on s and t."""
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        s_o, s_d, s_oo, s_od, n = (np.float64(v) for v in (s_o, s_d, s_oo, s_od, n))
        den = s_oo - (s_o * s_o) / n
        num = s_od - (s_o * s_d) / n
        s64 = num / den
        t64 = (s_d - s64 * s_o) / n
        return s64, t64, bool(n >= 2 and den > FLOOR * s_oo)


def loss64(out, tgt, masked):
    """((loss, valid fraction, mean scale, mean shift), gradient [b, npix], s [b], t [b], flag [b], n [b]) in float64."""
    o, d = np.asarray(out, np.float64), np.asarray(tgt, np.float64)
    b, npix = o.shape
    cnt = counting(d, masked)
    n = cnt.sum(axis=1)
    poisoned = poisoned_rows(o, d, cnt, masked)
    s, t, flag = np.zeros(b), np.zeros(b), np.full(b, DEGENERATE)
    per, g = np.zeros(b), np.zeros((b, npix))
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for i in range(b):
            if poisoned[i]:
                s[i] = t[i] = per[i] = np.nan
                flag[i] = POISONED
                g[i] = np.nan
                continue
            if n[i] == 0:
                continue
            oc, dc = o[i][cnt[i]], d[i][cnt[i]]
            s64, t64, ok = solve(oc.sum(), dc.sum(), (oc * oc).sum(), (oc * dc).sum(), n[i])
            if ok and np.isfinite(F(s64)) and np.isfinite(F(t64)):
                s[i], t[i], flag[i] = s64, t64, FITTED
            else:
                t[i] = dc.sum() / n[i]
            r = s[i] * oc + t[i] - dc
            h = 0.5 * npix / n[i] if masked else 0.5
            per[i] = h * (r * r).sum()
            if flag[i] == FITTED:
                g[i][cnt[i]] = s[i] * r * ((npix / n[i] if masked else 1.0) / b)
        losses = (per.sum() / b, n.sum() / (b * npix) if masked else 1.0, s.sum() / b, t.sum() / b)
    return losses, g, s, t, flag, n


def literal_loss(out, tgt, masked):
    """loss[0] as a torch float64 scalar; the scale and shift of a fitted sample come from solving the normal equations of [o 1] with torch.linalg.solve, so
    autograd differentiates through the fit.  A sample with fewer than two counting pixels or a constant output (den at or
    below the floor) is degenerate: s = 0, t = mean d, constants."""
    import torch
    b, npix = out.shape
    cnt = torch.isfinite(tgt) if masked else torch.ones_like(tgt, dtype=torch.bool)
    total = out.new_zeros(())
    for i in range(b):
        n = int(cnt[i].sum())
        if n == 0:
            continue
        o, d = out[i][cnt[i]], tgt[i][cnt[i]]
        soo = float((o * o).sum().detach())
        den = soo - float(o.sum().detach()) ** 2 / n
        if n >= 2 and den > FLOOR * soo:
            a = torch.stack([o, torch.ones_like(o)], dim=1)
            st = torch.linalg.solve(a.T @ a, a.T @ d)                   # the normal equations, differentiated through
            r = st[0] * o + st[1] - d
        else:
            r = d.mean().detach() - d
        total = total + (0.5 * npix / n if masked else 0.5) * (r * r).sum()
    return total / b


def _tree(v):
    """Lane 0 of v[l] += v[l + off], off = 32 .. 1, over the last axis of 64."""
    for off in (32, 16, 8, 4, 2, 1):
        v = v[..., :off] + v[..., off:2 * off]
    return v[..., 0]


def _partition_sum(values, dtype):
    """values [b, npix] (what does not count is +0) summed per sample in the header's order, in `dtype`."""
    b, npix = values.shape
    chunk = ((npix + PARTS - 1) // PARTS + 3) & ~3
    rounds = (chunk + 1023) // 1024
    grid = np.zeros((b, PARTS, rounds * 1024), dtype)
    for part in range(PARTS):
        lo, hi = min(npix, part * chunk), min(npix, (part + 1) * chunk)
        grid[:, part, :hi - lo] = values[:, lo:hi]
    grid = grid.reshape(b, PARTS, rounds, 256, 4)
    acc = np.zeros((b, PARTS, 256), dtype)
    for r in range(rounds):
        for u in range(4):
            acc = acc + grid[:, :, r, :, u]
    waves = _tree(acc.reshape(b, PARTS, 4, 64))
    parts = ((waves[..., 0] + waves[..., 1]) + waves[..., 2]) + waves[..., 3]
    total = np.zeros(b, dtype)
    for part in range(PARTS):
        total = total + parts[:, part]
    return total


def loss32(out, tgt, masked):
    """The same values in the arithmetic, the order and the partition include/a3d_ssi.h states: losses float32 [4], gradient
    float32, s, t float32 [b], flag, n."""
    o, d = np.asarray(out, F), np.asarray(tgt, F)
    b, npix = o.shape
    cnt = counting(d, masked)
    n = cnt.sum(axis=1)
    poisoned = poisoned_rows(o, d, cnt, masked)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        o64 = np.where(cnt, o, F(0)).astype(np.float64)
        d64 = np.where(cnt, d, F(0)).astype(np.float64)
        s_o, s_d = _partition_sum(o64, np.float64), _partition_sum(d64, np.float64)
        s_oo, s_od = _partition_sum(o64 * o64, np.float64), _partition_sum(o64 * d64, np.float64)
        s, t, flag = np.zeros(b, F), np.zeros(b, F), np.full(b, DEGENERATE)
        for i in range(b):
            if poisoned[i]:
                s[i] = t[i] = np.nan
                flag[i] = POISONED
            elif n[i] >= 1:
                s64, t64, ok = solve(s_o[i], s_d[i], s_oo[i], s_od[i], n[i])
                if ok and np.isfinite(F(s64)) and np.isfinite(F(t64)):
                    s[i], t[i], flag[i] = F(s64), F(t64), FITTED
                else:
                    t[i] = F(s_d[i] / np.float64(n[i]))
        q = ((s[:, None] * o).astype(F) + t[:, None]).astype(F)
        r = (q - np.where(cnt, d, F(0))).astype(F)
        rr = np.where(cnt, (r * r).astype(F), F(0)).astype(F)
        S = _partition_sum(rr, F)
        nn = np.maximum(n, 1).astype(np.float64)
        h = (0.5 * npix / nn).astype(F) if masked else np.full(b, 0.5, F)
        per = np.where(n > 0, (h * S).astype(F), F(0)).astype(F)
        l0, l2, l3 = F(0), F(0), F(0)
        for i in range(b):
            l0, l2, l3 = F(l0 + per[i]), F(l2 + s[i]), F(l3 + t[i])
        losses = np.array([F(l0 / F(b)), F(n.sum() / (b * npix)) if masked else F(1), F(l2 / F(b)), F(l3 / F(b))], F)
        rn = (npix / nn).astype(F) if masked else np.ones(b, F)
        k = (F(F(1) / F(b)) * rn).astype(F)[:, None]
        g = ((s[:, None] * r).astype(F) * k).astype(F)
        g = np.where(cnt & (flag == FITTED)[:, None], g, F(0))
        g = np.where(poisoned[:, None], F(np.nan), g).astype(F)
    return losses, g, s, t, flag, n


def rel(x, ref, scale=None):
    x, ref = float(x), float(ref)
    scale = abs(ref) if scale is None else float(scale)
    return 0.0 if x == ref else abs(x - ref) / scale if scale else float('inf')


def grad_err(g, g64):
    """The worst per-sample ||g - g64||inf / ||g64||inf; a sample whose reference row is zero must be zero (then 0, else inf)."""
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    worst = 0.0
    for row, ref in zip(g, g64):
        top = np.abs(ref).max(initial=0.0)
        diff = np.abs(row - ref).max(initial=0.0)
        worst = max(worst, 0.0 if diff == 0 else diff / top if top else float('inf'))
    return worst


def errors(losses, g, ref):
    """(loss, mean scale, mean shift, gradient) errors of `losses`, `g` against ref = loss64(...)."""
    l64, g64, s64, t64 = ref[:4]
    b = len(s64)
    return (rel(losses[0], l64[0]), rel(losses[2], l64[2], np.abs(s64).sum() / b), rel(losses[3], l64[3], np.abs(t64).sum() / b),
            grad_err(g, g64))


def bound(out, tgt, masked):
    """(loss64's result, loss bound, scale bound, shift bound, gradient bound): 8 x what loss32 shows against loss64 on these
    inputs."""
    ref = loss64(out, tgt, masked)
    l32, g32 = loss32(out, tgt, masked)[:2]
    return (ref,) + tuple(8 * e for e in errors(l32, g32, ref))


def case(b, npix, seed, masked):
    """(out, tgt) float32 [b, npix]: tests/berhu_ref.py's generator.  Targets uniform in (0.05, 1); outputs the target plus a
    normal error of 0.3 (den / S_oo is then about 0.3, far from the degenerate floor).  masked: holes (NaN, a few inf) as a run
    and a sprinkle, their outputs untouched, and with b >= 3 the middle sample without a finite target at all."""
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
    """Whole numbers for which every operation of the header is exact.  Every other pixel is a hole that carries a large error.
    The counting pixels come in runs of four with one output value v per run, the values in pairs (v, 8 - v) with v in 1..7
    (an odd run out holds 4), shuffled: their mean is 4, so S_o = 4 n and both divisions by n in the fit are exact.
    d = 2 o + 3 + e with e = (+k, -k, +k, -k) over a run, k in 0..3: sum e = sum e o = 0, so s64 = 2.0 and t64 = 3.0 exactly,
    r = -e, r_n = 2 and h = 1 (exact_conditions asserts all of it)."""
    assert npix % 8 == 0 and npix >= 32
    rng = np.random.default_rng(seed)
    runs = npix // 8
    o, t = np.full((b, npix), 64, F), np.full((b, npix), np.nan, F)
    for i in range(b):
        v = rng.integers(1, 8, runs // 2)
        v[0] = 1                                                        # the pair (1, 7): the output is not constant
        vals = np.concatenate([v, 8 - v, np.full(runs % 2, 4)])
        k = rng.integers(0, 4, runs)
        k[:4] = (0, 1, 2, 3)
        order = rng.permutation(runs)
        vals, k = vals[order], k[order]
        oc = np.repeat(vals, 4)
        e = np.repeat(k, 4) * np.tile([1, -1, 1, -1], runs)
        o[i, 0::2] = oc
        t[i, 0::2] = 2 * oc + 3 + e
    return o, t


def exact_conditions(o, t):
    """What makes integer_case exact at b in {1, 2, 4}: the fit is (2, 3) in float64 already, the residuals are whole numbers
    up to 3, r_n = 2, h = 1, b a power of two, and every sum a whole number far below 2^24."""
    b, npix = o.shape
    cnt = np.isfinite(t)
    assert (cnt.sum(axis=1) * 2 == npix).all() and b & (b - 1) == 0 and b <= 4
    losses, g, s, tt, flag, n = loss32(o, t, 1)
    for i in range(b):
        oc, dc = o[i][cnt[i]].astype(np.float64), t[i][cnt[i]].astype(np.float64)
        assert (oc == np.round(oc)).all() and (dc == np.round(dc)).all()
        s64, t64, ok = solve(oc.sum(), dc.sum(), (oc * oc).sum(), (oc * dc).sum(), n[i])
        assert s64 == 2.0 and t64 == 3.0 and ok
        r = 2 * oc + 3 - dc
        assert (r == np.round(r)).all() and np.abs(r).max() == 3 and (r * r).sum() < 2 ** 22
    assert (s == 2).all() and (tt == 3).all() and (flag == FITTED).all()
    assert F(0.5 * npix / n[0]) == 1 and F(npix / n[0]) == 2
