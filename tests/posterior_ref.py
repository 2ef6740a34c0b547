"""References of a3dc_crf_band_posterior (include/a3d_posterior.h) and the bounds its GPU test holds the kernel to
(tests/test_posterior_cpu.py, tests/test_gpu_posterior.py).

The field is y ~ N(mu, Sigma), Sigma = A^-1 / 2, mu = A^-1 z, A = I + D - R from the pair weights (tests/crf_band_ref.py has
the scatter).  O: the superpixels whose y is finite, M: the others.

post64   float64 from the COVARIANCE form, which shares no algebra with the kernel's precision form:
             mean_M = mu_M + Sigma_MO Sigma_OO^-1 (y_O - mu_O),   cov = Sigma_MM - Sigma_MO Sigma_OO^-1 Sigma_OM
         -> mean (y on O), var (diag cov on M, 0 on O), mu.
prec64   float64 from the precision form on the dense A' (A with the observed rows and columns replaced by the identity's):
         what the kernel computes, without its band storage; tests/test_posterior_cpu.py holds it to post64.
post32   the kernel's own arithmetic in numpy float32 (no FMA), in its order, in the manner of crf_band_ref.nll32: the band
         storage scattered directly, the diagonal over every stored cell (columns ascending), the right-hand side
         z_i - sum over observed neighbours of (-r_ij) y_j in the same column order, the masked cells dropped afterwards,
         right-looking L D L^T with the forward solve in its steps, the division by the pivots, the column sweep, the
         Takahashi recurrence row by row with its eight partial sums and the 32-lane butterfly for the diagonal.

Bounds.  The house rule (tests/crf_band_ref.py): bound(case, mask) = 8 x the error of post32 against post64 on the same
inputs, the margin for the device's division and summation order, and never less than one ulp (2^-23); no figure comes
from the kernel.  Error measure per image, for mean and for var: ||x - x64||inf / ||x64||inf over M (0 where M is empty).

Masks (obs [B, n] bool; the grid is rows x cols with cols = the case's band, a chain counts as one of `band` columns):
    none      nothing observed                      all       everything observed
    row       row 1 hidden (indices band .. 2 band - 1)
    one       a single observed superpixel, the last left-side superpixel of the pair lists
    checker   (row + col) even observed
    random    30 % hidden, drawn per image, so the masks differ within the batch
    interior  only the first left-side superpixel of the pair lists hidden (on a grid it has four pairs)

What tests/test_gpu_posterior.py printed on an MI355X, worst image per case: kernel error / bound (the bound is the CPU's:
8 x post32's error, floored at 1.19e-07).  The kernel reproduced post32's own error to three digits in every case (ratio
0.12 = 1 / 8 or below):
    3x4     none      mean  9.18e-08 / 7.35e-07  var  5.72e-08 / 4.58e-07
    3x4     all       mean         0 / 1.19e-07  var         0 / 1.19e-07
    3x4     row       mean   1.6e-07 / 1.28e-06  var     4e-08 / 3.2e-07
    3x4     one       mean  5.31e-08 / 4.25e-07  var  2.05e-08 / 1.64e-07
    3x4     checker   mean  6.71e-08 / 5.37e-07  var  2.05e-08 / 1.64e-07
    3x4     random    mean  3.79e-08 / 3.03e-07  var  8.32e-09 / 1.19e-07
    3x4     interior  mean  2.91e-08 / 2.33e-07  var  4.95e-08 / 3.96e-07
    6x8     none      mean  2.92e-07 / 2.34e-06  var  8.84e-08 / 7.08e-07
    6x8     all       mean         0 / 1.19e-07  var         0 / 1.19e-07
    6x8     row       mean  1.92e-07 / 1.54e-06  var  3.93e-08 / 3.14e-07
    6x8     one       mean  3.74e-07 / 3e-06     var   1.1e-07 / 8.78e-07
    6x8     checker   mean  1.07e-07 / 8.58e-07  var  2.91e-08 / 2.33e-07
    6x8     random    mean  1.18e-07 / 9.41e-07  var  2.61e-08 / 2.09e-07
    6x8     interior  mean  1.36e-07 / 1.09e-06  var  2.74e-08 / 2.19e-07
    5x13    none      mean  2.24e-07 / 1.79e-06  var  1.93e-07 / 1.54e-06
    5x13    all       mean         0 / 1.19e-07  var         0 / 1.19e-07
    5x13    row       mean  9.02e-08 / 7.22e-07  var  8.01e-08 / 6.4e-07
    5x13    one       mean  1.85e-07 / 1.48e-06  var  1.93e-07 / 1.54e-06
    5x13    checker   mean  9.86e-08 / 7.89e-07  var  4.95e-08 / 3.96e-07
    5x13    random    mean  1.01e-07 / 8.04e-07  var  3.57e-08 / 2.86e-07
    5x13    interior  mean  7.86e-08 / 6.29e-07  var  1.52e-08 / 1.21e-07
    12x16   none      mean  4.06e-07 / 3.25e-06  var  1.22e-07 / 9.74e-07
    12x16   all       mean         0 / 1.19e-07  var         0 / 1.19e-07
    12x16   row       mean  1.68e-07 / 1.34e-06  var  8.01e-08 / 6.41e-07
    12x16   one       mean   3.7e-07 / 2.96e-06  var  1.22e-07 / 9.74e-07
    12x16   checker   mean  1.29e-07 / 1.03e-06  var  5.72e-08 / 4.58e-07
    12x16   random    mean  1.42e-07 / 1.13e-06  var  5.05e-08 / 4.04e-07
    12x16   interior  mean  1.99e-08 / 1.59e-07  var  4.05e-08 / 3.24e-07
    3x32    none      mean  1.65e-07 / 1.32e-06  var  1.39e-07 / 1.11e-06
    3x32    all       mean         0 / 1.19e-07  var         0 / 1.19e-07
    3x32    row       mean  1.71e-07 / 1.37e-06  var  1.04e-07 / 8.32e-07
    3x32    one       mean  1.65e-07 / 1.32e-06  var  1.39e-07 / 1.11e-06
    3x32    checker   mean   9.6e-08 / 7.68e-07  var  6.42e-08 / 5.14e-07
    3x32    random    mean  8.44e-08 / 6.76e-07  var   7.7e-08 / 6.16e-07
    3x32    interior  mean  8.05e-08 / 6.44e-07  var  4.15e-08 / 3.32e-07
    24x32   none      mean  5.76e-07 / 4.61e-06  var  1.25e-07 / 1e-06
    24x32   all       mean         0 / 1.19e-07  var         0 / 1.19e-07
    24x32   row       mean  1.64e-07 / 1.32e-06  var  4.72e-08 / 3.78e-07
    24x32   one       mean  5.76e-07 / 4.61e-06  var  1.67e-07 / 1.34e-06
    24x32   checker   mean  1.35e-07 / 1.08e-06  var  6.01e-08 / 4.81e-07
    24x32   random    mean  1.67e-07 / 1.34e-06  var  6.01e-08 / 4.81e-07
    24x32   interior  mean  1.03e-07 / 8.2e-07   var  3.26e-08 / 2.61e-07
    8x8     none      mean  2.17e-07 / 1.73e-06  var  1.09e-07 / 8.7e-07
    8x8     all       mean         0 / 1.19e-07  var         0 / 1.19e-07
    8x8     row       mean  1.65e-07 / 1.32e-06  var  8.17e-08 / 6.54e-07
    8x8     one       mean  2.18e-07 / 1.74e-06  var  8.87e-08 / 7.1e-07
    8x8     checker   mean   1.5e-07 / 1.2e-06   var  5.71e-08 / 4.57e-07
    8x8     random    mean  1.87e-07 / 1.5e-06   var  6.24e-08 / 4.99e-07
    8x8     interior  mean  6.03e-08 / 4.82e-07  var  6.41e-08 / 5.12e-07
    chain1  none      mean  1.52e-07 / 1.22e-06  var  1.61e-07 / 1.29e-06
    chain1  all       mean         0 / 1.19e-07  var         0 / 1.19e-07
    chain1  row       mean  6.37e-08 / 5.1e-07   var  5.16e-08 / 4.13e-07
    chain1  one       mean  1.19e-07 / 9.56e-07  var   1.6e-07 / 1.28e-06
    chain1  checker   mean   1.3e-07 / 1.04e-06  var  9.13e-08 / 7.3e-07
    chain1  random    mean  1.66e-07 / 1.33e-06  var   7.7e-08 / 6.16e-07
    chain1  interior  mean  4.44e-08 / 3.55e-07  var  3.05e-08 / 2.44e-07
    chain32 none      mean  1.12e-07 / 8.97e-07  var   1.2e-07 / 9.61e-07
    chain32 all       mean         0 / 1.19e-07  var         0 / 1.19e-07
    chain32 row       mean  7.91e-08 / 6.33e-07  var  6.97e-08 / 5.58e-07
    chain32 one       mean  1.12e-07 / 8.97e-07  var   1.2e-07 / 9.61e-07
    chain32 checker   mean  7.51e-08 / 6.01e-07  var  6.81e-08 / 5.45e-07
    chain32 random    mean  8.86e-08 / 7.09e-07  var  6.89e-08 / 5.51e-07
    chain32 interior  mean  1.26e-08 / 1.19e-07  var  4.48e-08 / 3.58e-07
"""
import functools

import numpy as np

import crf_band_ref as R

F = np.float32
ULP = float(np.finfo(F).eps)                  # 2^-23
MASKS = ['none', 'all', 'row', 'one', 'checker', 'random', 'interior']
HIDDEN = 0.3                                  # 'random'


@functools.lru_cache(maxsize=None)
def mask(case, name):
    """obs [B, n] bool, read-only."""
    left, right, n, band = R.pairs(case)
    B = R.batch_of(case)
    obs = np.ones((B, n), bool)
    idx = np.arange(n)
    if name == 'none':
        obs[:] = False
    elif name == 'row':
        obs[:, band:2 * band] = False
    elif name == 'one':
        obs[:] = False
        obs[:, left[-1]] = True
    elif name == 'checker':
        obs[:] = ((idx // band + idx % band) % 2 == 0)[None, :]
    elif name == 'random':
        rng = np.random.default_rng(9000 + R.CASES.index(case))
        obs = rng.random((B, n)) >= HIDDEN
        assert any((obs[0] != obs[b]).any() for b in range(1, B))
    elif name == 'interior':
        obs[:, left[0]] = False
    else:
        assert name == 'all'
    obs.setflags(write=False)
    return obs


@functools.lru_cache(maxsize=None)
def draw(case, name):
    """(z, y [B, n] with NaN where the mask hides, r [B, npairs]) float32, read-only: crf_band_ref's draw, punched."""
    z, y, r = R.draw(case)
    y = np.where(mask(case, name), y, F(np.nan)).astype(F)
    y.setflags(write=False)
    return z, y, r


# ------------------------------------------------------------------------------------------------ float64
def post64(z, y, r, left, right):
    """The covariance form -> dict(mean [B, n], var [B, n], mu [B, n], obs [B, n]) in float64."""
    z, y, r = (np.asarray(a, np.float64) for a in (z, y, r))
    B, n = z.shape
    left, right = np.asarray(left, np.int64), np.asarray(right, np.int64)
    mean, var, mu_all = np.zeros((B, n)), np.zeros((B, n)), np.zeros((B, n))
    obs = np.isfinite(y)
    for b in range(B):
        A = R.matrix(r[b], n, left, right)
        sigma = np.linalg.inv(A) / 2
        mu = mu_all[b] = 2 * sigma @ z[b]
        O, M = obs[b], ~obs[b]
        mean[b, O] = y[b, O]
        if not M.any():
            continue
        if not O.any():
            mean[b], var[b] = mu, np.diag(sigma)
            continue
        s_mo, s_oo = sigma[np.ix_(M, O)], sigma[np.ix_(O, O)]
        mean[b, M] = mu[M] + s_mo @ np.linalg.solve(s_oo, y[b, O] - mu[O])
        var[b, M] = np.diag(sigma[np.ix_(M, M)] - s_mo @ np.linalg.solve(s_oo, s_mo.T))
    return dict(mean=mean, var=var, mu=mu_all, obs=obs)


def masked_matrix(A, obs):
    """A' and the selector of the right-hand side's observed part: A with the observed rows and columns replaced by the
    identity's."""
    Ap = A.copy()
    Ap[obs, :] = 0
    Ap[:, obs] = 0
    Ap[obs, obs] = 1
    return Ap


def prec64(z, y, r, left, right):
    """The precision form on the dense A' -> dict(mean, var, logdet [B]) in float64."""
    z, y, r = (np.asarray(a, np.float64) for a in (z, y, r))
    B, n = z.shape
    mean, var, logdet = np.zeros((B, n)), np.zeros((B, n)), np.zeros(B)
    obs = np.isfinite(y)
    for b in range(B):
        A = R.matrix(r[b], n, left, right)
        O = obs[b]
        y0 = np.where(O, y[b], 0.0)
        rhs = np.where(O, 0.0, z[b] - A @ y0)                  # -A_MO y_O = + sum over observed neighbours of r_ij y_j
        Ap = masked_matrix(A, O)
        x = np.linalg.solve(Ap, rhs)
        mean[b] = np.where(O, y[b], x)
        var[b] = np.where(O, 0.0, 0.5 * np.diag(np.linalg.inv(Ap)))
        logdet[b] = np.linalg.slogdet(Ap)[1]
    return dict(mean=mean, var=var, logdet=logdet, obs=obs)


# ------------------------------------------------------------------------------------------------ float32
def post32(z, y, r, left, right, band, want_var=True):
    """The kernel's arithmetic in numpy float32, all images at once -> dict(mean, var or None, nobs, status)."""
    z, r = (np.ascontiguousarray(a, F) for a in (z, r))
    B, n = z.shape
    y = np.full((B, n), np.nan, F) if y is None else np.ascontiguousarray(y, F)
    left, right = np.asarray(left, np.int64), np.asarray(right, np.int64)
    live = R.owners(left, right)
    obs = np.isfinite(y)
    GROUPS = R.GROUPS
    with np.errstate(all='ignore'):
        S = np.zeros((B, n, band + 1), F)
        for q in np.flatnonzero(live):
            lo, d = min(left[q], right[q]), abs(left[q] - right[q])
            S[:, lo, d] = F(0) - r[:, q]
        rs = np.zeros((B, n), F)
        acc = z.copy()
        for e in range(band, 0, -1):                             # columns i - band .. i - 1
            if e < n:
                rs[:, e:] = rs[:, e:] + S[:, :n - e, e]
                acc[:, e:] = acc[:, e:] - np.where(obs[:, :n - e], S[:, :n - e, e] * y[:, :n - e], F(0))
        for d in range(1, band + 1):                             # columns i + 1 .. i + band
            rs = rs + S[:, :, d]
            if d < n:
                acc[:, :n - d] = acc[:, :n - d] - np.where(obs[:, d:], S[:, :n - d, d] * y[:, d:], F(0))
        S[:, :, 0] = np.where(obs, F(1), F(1) - rs)
        zv = np.where(obs, F(0), acc).astype(F)
        for d in range(1, min(band, n - 1) + 1):                 # A -> A'
            kill = obs[:, :n - d] | obs[:, d:]
            S[:, :n - d, d] = np.where(kill, F(0), S[:, :n - d, d])
        for k in range(n):
            w = min(band, n - 1 - k)
            if w == 0:
                continue
            col = S[:, k, :].copy()
            li = col[:, 1:w + 1] / col[:, 0:1]
            for j in range(1, w + 1):
                S[:, k + j, 0:w - j + 1] = S[:, k + j, 0:w - j + 1] - li[:, j - 1:w] * col[:, j:j + 1]
            zv[:, k + 1:k + w + 1] = zv[:, k + 1:k + w + 1] - li * zv[:, k:k + 1]
        p = S[:, :, 0].copy()
        ok = ((p > 0) & (p < np.inf)).all(axis=1)
        zv = zv / p
        S[:, :, 1:] = S[:, :, 1:] / p[:, :, None]
        for k in range(n - 1, 0, -1):
            d = np.arange(1, min(band, k) + 1)
            zv[:, k - d] = zv[:, k - d] - S[:, k - d, d] * zv[:, k:k + 1]
        ok &= np.isfinite(zv).all(axis=1)
        var = None
        if want_var:
            lanes = np.arange(32)
            for i in range(n - 1, -1, -1):                       # Takahashi, in place
                w = min(band, n - 1 - i)
                col = S[:, i, :].copy()
                prod = np.zeros((B, 32), F)
                if w > 0:
                    d = np.arange(1, w + 1)
                    part = np.zeros((GROUPS, B, w), F)
                    for m in range(1, w + 1):
                        rows = np.where(m <= d, i + m, i + d)
                        g = (m - 1) % GROUPS
                        part[g] = part[g] + col[:, m:m + 1] * S[:, rows, np.abs(d - m)]
                    a = part[0]
                    for g in range(1, GROUPS):
                        a = a + part[g]
                    zij = F(0) - a
                    prod[:, :w] = col[:, 1:w + 1] * zij
                    S[:, i, 1:w + 1] = zij
                for off in (16, 8, 4, 2, 1):
                    prod = prod + prod[:, lanes ^ off]
                S[:, i, 0] = F(1) / col[:, 0] - prod[:, 0]
            v = F(0.5) * S[:, :, 0]
            ok &= (obs | ((v > 0) & (v < np.inf))).all(axis=1)
            var = np.where(obs, F(0), v).astype(F)
            var[~ok] = np.nan
        mean = np.where(obs, y, zv).astype(F)
        mean[~ok] = np.nan
    return dict(mean=mean, var=var, nobs=obs.sum(axis=1).astype(np.int32), status=(~ok).astype(np.int32))


# ------------------------------------------------------------------------------------------------ errors and bounds
def rel_inf_hidden(x, x64, obs):
    """Per image ||x - x64||inf / ||x64||inf over the hidden superpixels; 0 where there is none."""
    x = np.asarray(x, np.float64)
    out = np.zeros(len(x))
    for b in range(len(x)):
        M = ~obs[b]
        if M.any():
            out[b] = (np.maximum(np.abs(x[b, M] - x64[b, M]) - R.FLT_MIN, 0).max()
                      / max(np.abs(x64[b, M]).max(), R.FLT_MIN))
    return out


def errors(got, ref):
    """Per-image (mean, var) errors of a float32 result against post64's; a missing var counts as exact."""
    e_var = rel_inf_hidden(got['var'], ref['var'], ref['obs']) if got.get('var') is not None else np.zeros(len(ref['obs']))
    return rel_inf_hidden(got['mean'], ref['mean'], ref['obs']), e_var


def bound_of(z, y, r, left, right, band):
    e = errors(post32(z, y, r, left, right, band), post64(z, y, r, left, right))
    return tuple(max(8 * float(x.max()), ULP) for x in e)


@functools.lru_cache(maxsize=None)
def reference(case, name):
    left, right, _, _ = R.pairs(case)
    return post64(*draw(case, name), left, right)


@functools.lru_cache(maxsize=None)
def restatement(case, name):
    left, right, _, band = R.pairs(case)
    return post32(*draw(case, name), left, right, band)


@functools.lru_cache(maxsize=None)
def measured(case, name):
    """The worst image's (mean, var) error of post32 against post64."""
    return tuple(float(x.max()) for x in errors(restatement(case, name), reference(case, name)))


def bound(case, name):
    """(mean, var): 8 x measured, never below one ulp."""
    return tuple(max(8 * m, ULP) for m in measured(case, name))


if __name__ == '__main__':                   # the table of the docstring
    for c in R.CASES:
        print('    ' + f'{c:8s}' + '  '.join(f'{m} {measured(c, m)[0]:.1e}/{measured(c, m)[1]:.1e}' for m in MASKS))
