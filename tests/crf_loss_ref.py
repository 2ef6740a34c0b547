"""References of a3d_crf_loss (loss_part, src/models.py:129-177) for any superpixel grid, explicit pair lists and any
epsilon, and the bounds its GPU tests hold the kernel to (tests/test_crf_loss_cpu.py, tests/test_gpu_crf_loss.py,
tests/test_gpu_dcnf.py).

loss64     the float64 restatement on A = crf_map_ref.matrix (pairs scattered in order, a later pair overwrites an
           earlier one), A a constant for the gradient: (mean, per_image, dz, det).
loss32     the same formulas in numpy float32 in the kernel's order of operations (no FMA: crf.hip is compiled without
           contraction): sequential row sums, the 64-lane butterfly sums, LU with partial pivoting where the largest
           |U[i][k]| wins and the lowest row wins a tie, serial back substitution.  Only expf / logf / sqrtf are numpy's,
           not the device's.  (mean, per_image, dz, det, swaps), swaps the row exchanges per image.

Bounds.  For every (grid, regime) and the batches 1, 5, 64 and 130 of draw(), err_loss is the per-image relative error
of loss32 against loss64 and err_dz the per-image ||dz32 - dz64||inf / ||dz64||inf (dz64 carrying the same 1/B).  The
kernel is held to 8 x the worst such figure over the regime's draws, the margin tests/test_gpu_crf_map.py leaves for
another summation order.  The measured figures depend on numpy's float32 exp / log / sqrt and on its random streams; in
the 'reference' rows of the 6x8 and 8x8 grids the loss is pinned at -log(eps), every image has the same float32 loss
and the "worst" loss figure is the rounding of that one number, so tests/test_crf_loss_cpu.py holds those two entries
from below only.  tests/test_crf_loss_cpu.py recomputes the table and pins the constants to it.

  measured (float32 restatement vs float64)          bound = 8 x           kernel on an MI355X reached
  grid  regime        worst loss   worst dz          loss       dz         loss       dz
  6x8   reference     6.41e-08     5.45e-06          5.2e-07    4.4e-05    1.26e-07   5.45e-06
  6x8   unsaturated   7.03e-07     3e-06             5.7e-06    2.5e-05    6.46e-07   3e-06
  6x8   pivoting      0.00113      0.000257          0.0091     0.0021     0.00113    0.000257
  3x4   reference     2.92e-07     1.97e-06          2.4e-06    1.6e-05    3.74e-07   1.97e-06
  3x4   unsaturated   3.55e-07     1.01e-06          2.9e-06    8.2e-06    3.74e-07   1.01e-06
  3x4   pivoting      8.95e-06     3.04e-06          7.2e-05    2.5e-05    9.01e-06   3.04e-06
  8x8   reference     6.21e-08     6.29e-06          5e-07      5.1e-05    1.3e-07    6.18e-06
  8x8   unsaturated   7.83e-07     3.42e-06          6.3e-06    2.8e-05    8.01e-07   3.42e-06
  8x8   pivoting      1.58e-06     8.81e-06          1.3e-05    7.1e-05    1.65e-06   8.81e-06

6x8 'pivoting': both worst figures are one image each of the batch of 64 (cond_inf(A) = 1.4e4 with a loss of 0.23, and
cond_inf(A) = 2.3e3); every other image of the regime stays below 1.1e-5 and 1.4e-5.  The kernel reproduces the
restatement's worst figures to three digits wherever the LU dominates, which is what the restatement is for.

(8, 8) 'stiff' overflows float32's determinant (2e80): the expectation there is loss32's answer itself (its inf / NaN
pattern exactly, finite values within STIFF_BOUND of it), not float64's.

Broken-kernel runs on an MI355X (scratch builds with one defect each, never committed) against
tests/test_gpu_crf_loss.py and against the parent commit's tests/test_gpu_dcnf.py with tests/test_gpu_eval_dcnf.py and
tests/test_gpu_crf_map.py; the parent's tests passed against all three (58 of 58 each time):
  * `det = -det` dropped: test_loss_and_gradient_match_float64 fails in 10 of the 12 'pivoting' cases (every batch that
    holds an image with an odd number of exchanges: all but batch 1 on 6x8 and 3x4) and
    test_a_negative_determinant_is_nan_and_only_that fails; 11 of 47.
  * the pivot taken without the row exchange: the same two tests, 11 of the 12 'pivoting' cases (all but 6x8 batch 1)
    and the negative-determinant test; 12 of 47.
  * `eps * zsum * zsum` dropped from g: both cases of test_a_large_epsilon_makes_its_terms_count, which is there for
    it, fail; and at eps = 1e-7, where the term is 6e-5 of g on the larger grids, 18 cases of
    test_loss_and_gradient_match_float64 fail on dz or the loss: every 'reference' case and all but one 'unsaturated'
    case of 6x8 and 8x8, three 'pivoting' cases; no 'reference' or 'unsaturated' case of 3x4, where (sum z)^2 is a
    sixteenth of that; 20 of 47.
"""
import functools

import numpy as np

import crf_map_ref as M

U = M.U
F = np.float32
FLT_MIN = float(np.finfo(np.float32).tiny)
GRIDS = [(6, 8), (3, 4), (8, 8)]
BATCHES = [1, 5, 64, 130]
REGIMES = {'reference': (-0.1, 0.7), 'unsaturated': (2.0, 2.3), 'indefinite': (-1.4, 1.4), 'stiff': (0.0, 50.0)}
ACCURACY_REGIMES = ['reference', 'unsaturated', 'pivoting']
EPSILON = 1e-7

# 8 x the measured worst, rounded up to two digits: {(rows, cols): {regime: (loss bound, dz bound)}}
BOUNDS = {
    (6, 8): {'reference': (5.2e-07, 4.4e-05), 'unsaturated': (5.7e-06, 2.5e-05), 'pivoting': (0.0091, 0.0021)},
    (3, 4): {'reference': (2.4e-06, 1.6e-05), 'unsaturated': (2.9e-06, 8.2e-06), 'pivoting': (7.2e-05, 2.5e-05)},
    (8, 8): {'reference': (5e-07, 5.1e-05), 'unsaturated': (6.3e-06, 2.8e-05), 'pivoting': (1.3e-05, 7.1e-05)},
}
STIFF_BOUND = BOUNDS[(8, 8)]['unsaturated']          # against loss32 where it is finite
# eps = 1e-4 on the 3x4 'unsaturated' draws of batch 5 and 64, where eps * (sum z)^2 is 2e-3 .. 7e-3 of g and u + eps is
# not u: measured 3.24e-07 (loss) and 8.69e-07 (dz); the kernel on an MI355X reached 4.13e-07 and 8.69e-07
LARGE_EPS, LARGE_EPS_BATCHES, LARGE_EPS_BOUND = 1e-4, [5, 64], (2.6e-06, 7.0e-06)


def pairs(rows, cols):
    return M.pairs(rows, cols)


# ------------------------------------------------------------------------------------------------ float64
def loss64(z, y, r, left, right, eps=EPSILON):
    """z, y [B, n], r [B, npairs] (float32 values are widened) -> (mean, per_image [B], dz [B, n], det [B])."""
    z, y, r = (np.asarray(a, np.float64) for a in (z, y, r))
    B, n = z.shape
    per, dz, det = np.zeros(B), np.zeros((B, n)), np.zeros(B)
    fac0 = np.pi ** (n / 2)
    with np.errstate(all='ignore'):
        for b in range(B):
            A = M.matrix(r[b], n, left, right)
            zb, yb = z[b], y[b]
            energy = yb @ A @ yb - 2 * (zb @ yb) + zb @ zb
            det[b] = np.linalg.det(A)
            try:
                w = np.linalg.solve(A, zb)
            except np.linalg.LinAlgError:                        # exactly singular
                w = np.full(n, np.nan)
            zsum = zb.sum()
            g = zb @ w + eps * zsum * zsum - zb @ zb
            fac = fac0 / (np.sqrt(det[b]) + eps)
            ex = np.exp(g)
            Z = fac * ex + eps
            u = np.exp(-energy) / Z
            per[b] = -np.log(u + eps)
            dE = -2 * yb + 2 * zb
            dg = 2 * w + 2 * eps * zsum - 2 * zb
            du = u * (-dE) - (u / Z) * (fac * ex * dg)
            dz[b] = (-du / (u + eps)) / B
    return per.mean(), per, dz, det


# ------------------------------------------------------------------------------------------------ float32
_LANES = np.arange(64)


def _wave_sum(v):
    """wave_sum_f of crf.hip over [B, 64] float32: every lane adds its partner's value, offsets 32, 16, ... 1."""
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, _LANES ^ off]
    return v[:, 0]


def _pad64(v):
    out = np.zeros((v.shape[0], 64), F)
    out[:, :v.shape[1]] = v
    return out


def loss32(z, y, r, left, right, eps=EPSILON):
    """The kernel's arithmetic in numpy float32, all images at once -> (mean, per_image, dz, det, swaps)."""
    z, y, r = (np.ascontiguousarray(a, F) for a in (z, y, r))
    B, n = z.shape
    eps, idx = F(eps), np.arange(B)
    with np.errstate(all='ignore'):
        R = np.zeros((B, n, n), F)
        for q in range(len(left)):
            R[:, left[q], right[q]] = r[:, q]
            R[:, right[q], left[q]] = r[:, q]
        rs = np.zeros((B, n), F)
        for j in range(n):
            rs = rs + R[:, :, j]
        A = -R                                                   # 0.f - R off the diagonal
        d = np.arange(n)
        A[:, d, d] = (F(1) + rs) - R[:, d, d]
        ay = np.zeros((B, n), F)
        for j in range(n):
            ay = ay + A[:, :, j] * y[:, j:j + 1]
        yAy, zy, zz, zsum = (_wave_sum(_pad64(v)) for v in (y * ay, z * y, z * z, z))
        energy = (yAy - F(2) * zy) + zz
        Um = np.concatenate([A, z[:, :, None]], axis=2)          # [A | z]
        det, swaps = np.ones(B, F), np.zeros(B, np.int64)
        for k in range(n):
            arg = k + np.argmax(np.abs(Um[:, k:, k]), axis=1)    # the first of equal maxima: the lowest row
            sw = arg != k
            tmp = Um[idx, k].copy()
            Um[idx, k] = Um[idx, arg]
            Um[idx, arg] = tmp
            det = np.where(sw, -det, det)
            swaps += sw
            piv = Um[:, k, k]
            det = det * piv
            f = Um[:, k + 1:, k] / piv[:, None]
            Um[:, k + 1:, k:] = Um[:, k + 1:, k:] - f[:, :, None] * Um[:, None, k, k:]
        w = np.zeros((B, n), F)
        for i in range(n - 1, -1, -1):
            s = Um[:, i, n].copy()
            for j in range(i + 1, n):
                s = s - Um[:, i, j] * w[:, j]
            w[:, i] = s / Um[:, i, i]
        zw = _wave_sum(_pad64(z * w))
        g = (zw + (eps * zsum) * zsum) - zz
        fac = F(np.pi ** (n / 2.0)) / (np.sqrt(det) + eps)
        ex = np.exp(g)
        Z = fac * ex + eps
        u = np.exp(-energy) / Z
        per = -np.log(u + eps)
        dE = F(-2) * y + F(2) * z
        dg = (F(2) * w + ((F(2) * eps) * zsum)[:, None]) - F(2) * z
        du = u[:, None] * (-dE) - (u / Z)[:, None] * ((fac * ex)[:, None] * dg)
        dz = (-du / (u + eps)[:, None]) * (F(1) / F(B))
    return mean32(per), per, dz, det, swaps


def mean32(per):
    """mean_kernel of crf.hip, bit for bit: lane i adds images i, i + 64, ... in order, the butterfly, / B."""
    per = np.asarray(per, F)
    s = np.zeros(64, F)
    with np.errstate(all='ignore'):
        for i in range(len(per)):
            s[i % 64] = s[i % 64] + per[i]
        return _wave_sum(s[None])[0] / F(len(per))


# ------------------------------------------------------------------------------------------------ draws and errors
def _zy(rng, batch, nsp):
    y = rng.random((batch, nsp)).astype(F)
    z = (y + 0.05 * rng.standard_normal((batch, nsp))).astype(F)
    return z, y


def seed_of(rows, cols, batch, regime):
    return 100000 * rows * cols + 100 * batch + (list(REGIMES) + ['pivoting']).index(regime)


@functools.lru_cache(maxsize=None)
def draw(rows, cols, batch, regime):
    """The inputs every test of this (grid, batch, regime) uses: (z, y, r) float32, read-only.  'reference' and
    'unsaturated' are the regimes of tests/test_gpu_dcnf.py; of the 'unsaturated' candidates only those whose float64
    loss is below 15.5 are kept (a large energy saturates an image whatever its determinant is).  'pivoting':
    'unsaturated' weights with six pairs (all of them on a grid that has fewer) set to uniform(-1.6, -0.9), keeping only
    images for which loss32 exchanges rows at least once, the float64 determinant is positive and the float64 loss is
    below 15.5."""
    left, right = pairs(rows, cols)
    nsp, npairs = rows * cols, len(left)
    rng = np.random.default_rng(seed_of(rows, cols, batch, regime))
    if regime not in ('unsaturated', 'pivoting'):
        lo, hi = REGIMES[regime]
        z, y = _zy(rng, batch, nsp)
        out = (z, y, rng.uniform(lo, hi, (batch, npairs)).astype(F))
    else:
        cand = 12 * batch + 40
        z, y = _zy(rng, cand, nsp)
        r = rng.uniform(*REGIMES['unsaturated'], (cand, npairs)).astype(F)
        if regime == 'pivoting':
            for b in range(cand):
                neg = rng.choice(npairs, min(6, npairs), replace=False)
                r[b, neg] = rng.uniform(-1.6, -0.9, len(neg)).astype(F)
        _, per, _, det = loss64(z, y, r, left, right)
        ok = per < 15.5
        if regime == 'pivoting':
            ok &= (loss32(z, y, r, left, right)[4] >= 1) & (det > 0)
        keep = np.flatnonzero(ok)[:batch]
        assert len(keep) == batch, f'{len(keep)} of {cand} candidates qualify, {batch} wanted'
        out = (z[keep], y[keep], r[keep])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def indefinite_batch(rows=6, cols=8):
    """Eight 'indefinite' images (r uniform in [-1.4, 1.4]) whose determinant is well away from 0: cond_inf(A) < 1000
    and the float32 LU's determinant within 1e-3 of float64's, so both agree on its sign.  Images 0, 2, 4, 6 have
    det < 0; 1, 3 have det > 0 after an odd number of row exchanges, 5, 7 after an even number.
    -> (z, y, r, det64, swaps)."""
    left, right = pairs(rows, cols)
    nsp = rows * cols
    rng = np.random.default_rng(seed_of(rows, cols, 8, 'indefinite'))
    z, y = _zy(rng, 400, nsp)
    r = rng.uniform(*REGIMES['indefinite'], (400, len(left))).astype(F)
    det = loss64(z, y, r, left, right)[3]
    _, _, _, det32, swaps = loss32(z, y, r, left, right)
    cond = np.array([M.cond_inf(M.matrix(r[b], nsp, left, right)) for b in range(400)])
    ok = (cond < 1000) & (np.abs(det32 / det - 1) < 1e-3)
    neg = np.flatnonzero(ok & (det < 0))[:4]
    odd = np.flatnonzero(ok & (det > 0) & (swaps % 2 == 1))[:2]
    even = np.flatnonzero(ok & (det > 0) & (swaps % 2 == 0) & (swaps > 0))[:2]
    assert len(neg) == 4 and len(odd) == 2 and len(even) == 2
    keep = np.array([neg[0], odd[0], neg[1], odd[1], neg[2], even[0], neg[3], even[1]])
    out = (z[keep], y[keep], r[keep], det[keep], swaps[keep])
    for a in out:
        a.setflags(write=False)
    return out


def errors(per, dz, per64, dz64):
    """Per-image relative loss error and ||.||inf-relative dz error of a float32 result against float64; a dz below the
    float32 normal range may have been flushed to 0."""
    per, dz = np.asarray(per, np.float64), np.asarray(dz, np.float64)
    e_loss = np.abs(per - per64) / np.abs(per64)
    e_dz = np.maximum(np.abs(dz - dz64) - FLT_MIN, 0).max(axis=1) / np.maximum(np.abs(dz64).max(axis=1), FLT_MIN)
    return e_loss, e_dz


@functools.lru_cache(maxsize=None)
def reference(rows, cols, batch, regime):
    """loss64 of draw(): computed once, shared, read-only."""
    out = loss64(*draw(rows, cols, batch, regime), *pairs(rows, cols))
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restatement(rows, cols, batch, regime):
    """loss32 of draw(): computed once, shared, read-only."""
    out = loss32(*draw(rows, cols, batch, regime), *pairs(rows, cols))
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def measured(rows, cols, regime):
    """(worst loss error, worst dz error) of loss32 against loss64 over the regime's draws."""
    worst = np.zeros(2)
    for batch in BATCHES:
        _, per32, dz32, _, _ = restatement(rows, cols, batch, regime)
        _, per64, dz64, _ = reference(rows, cols, batch, regime)
        e_loss, e_dz = errors(per32, dz32, per64, dz64)
        worst = np.maximum(worst, [e_loss.max(), e_dz.max()])
    return float(worst[0]), float(worst[1])


def measured_large_eps():
    worst = np.zeros(2)
    for batch in LARGE_EPS_BATCHES:
        args = (*draw(3, 4, batch, 'unsaturated'), *pairs(3, 4), LARGE_EPS)
        _, per64, dz64, _ = loss64(*args)
        worst = np.maximum(worst, [e.max() for e in errors(*loss32(*args)[1:3], per64, dz64)])
    return float(worst[0]), float(worst[1])


def bound(rows, cols, regime):
    b_loss, b_dz = BOUNDS[(rows, cols)][regime]
    return b_loss, b_dz
