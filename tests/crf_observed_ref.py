"""References of a3dv_crf_loss_observed and a3dv_superpixel_mean_valid (include/a3d_crf_valid.h), and the bounds their GPU
tests hold the kernels to (tests/test_crf_observed_cpu.py, tests/test_gpu_crf_observed.py,
tests/test_gpu_superpixel_valid.py, tests/test_gpu_dcnf_valid_train.py).  Pairs, draws, grids and the scatter semantics
(crf_map_ref.matrix: pairs in order, the last writer owns a cell) are crf_loss_ref's.

The field is y ~ N(mu, A^-1 / 2), mu = A^-1 z.  O = the superpixels whose target is finite, m = |O|, C = (A^-1)[O, O],
e = y_O - mu_O:    L = e^T C^-1 e + 1/2 log det C + (m / 2) log pi,    the batch objective sum_b L_b / B.

nll64        the literal definition in float64 from numpy.linalg on the sub-blocks (inv, slogdet, solve), and the closed
             forms  dz = -2 q / B,  dr_k = (2 (v^T q)(v^T mu) + (v^T q)^2 - 1/2 t^T C^-1 t) / B  with u = C^-1 e,
             q = A^-1 P^T u, v = e_l - e_r, t = (A^-1 v)[O]; 0 for a pair that a later pair overwrote.
literal_loss the same definition on torch float64 tensors, for autograd: the check of the closed forms that does not share
             their algebra (tests/test_crf_observed_cpu.py).
nll32        the kernel's own order of operations in numpy float32 (no FMA): [A | z | I] eliminated with the loss kernel's
             pivot rule, log det A the sequential sum of the logs of the pivots, mu and A^-1 back-substituted; then the
             missing rows and columns moved together, [A_MM | z_M - A_MO y_O | I] the same way; q = yhat - mu,
             L = (q^T A q + 0.5 (ld_M - ld_A)) + m * fl(log(pi) / 2), q^T A q by sequential row sums and the 64-lane
             butterfly;  dr_k = (((2 vq) vm + vq vq) - 0.5 (S_k(A^-1) - S_k(A_MM^-1))) / B.  Only logf is numpy's.

Bounds.  The rule of tests/test_gpu_crf_loss.py: per (grid, regime, mask), over the batches 1, 5 and 130 of
crf_loss_ref.draw(), the worst per-image error of nll32 against nll64; the kernel is held to 8 x that figure (the margin
for another summation order and the device's logf).  measured() computes the figures on the CPU when a test asks; no
figure comes from the kernel.  Error measures, per image:
  loss  |L - L64| / (|e^T C^-1 e| + |1/2 log det C| + (m / 2) log pi): L is a sum of terms of either sign (the log
        determinant is negative, the loss itself crosses 0 within the draws), so the scale is the size of its terms, not
        the size of their sum;
  dz    ||dz - dz64||inf / ||dz64||inf, crf_loss_ref.errors' measure;    dr    likewise, crf_pair_grad_ref.dr_errors'.
Regimes: 'reference' and 'unsaturated', where A is strictly diagonally dominant (r > -0.1 with at most four neighbours),
hence positive definite, for every image; the tests assert it in float64.  'pivoting' draws are indefinite in part and
have a test of their own.  With no superpixel observed every output is +0.0 exactly: no bound applies.

Observed on an MI355X (tests/test_gpu_crf_observed.py prints them): the kernel's worst error over the batches 1, 5, 130
beside the bound, which is 8 x the restatement's worst figure.  The kernel reproduces the restatement's own figures to
two or three digits nearly everywhere, which is what the restatement is for.  'one' (a single observed superpixel) leaves
dz as differences of nearly equal numbers: its figures are a hundred times the others', in float32 as on the device.
  grid regime       mask      loss: kernel / bound     dz: kernel / bound       dr: kernel / bound
  6x8  reference   all       8.1e-08  / 9.17e-07     1.19e-06 / 9.5e-06      5.5e-07  / 4.4e-06
  6x8  reference   interior  7.71e-08 / 6.95e-07     1.19e-06 / 9.5e-06      5.5e-07  / 4.4e-06
  6x8  reference   corner    8.16e-08 / 7.82e-07     1.19e-06 / 9.5e-06      5.5e-07  / 4.4e-06
  6x8  reference   row       1.31e-07 / 1.21e-06     1.2e-06  / 9.61e-06     5.5e-07  / 4.4e-06
  6x8  reference   one       2.42e-06 / 1.94e-05     0.000305 / 0.00244      2.57e-06 / 2.06e-05
  6x8  unsaturated all       1e-07    / 7.37e-07     9.3e-07  / 7.44e-06     2.74e-07 / 2.19e-06
  6x8  unsaturated interior  1.2e-07  / 8.24e-07     9.3e-07  / 7.44e-06     2.74e-07 / 2.19e-06
  6x8  unsaturated corner    9.76e-08 / 7.69e-07     9.3e-07  / 7.44e-06     2.74e-07 / 2.19e-06
  6x8  unsaturated row       1.34e-07 / 1.05e-06     9.3e-07  / 7.44e-06     3.12e-07 / 2.5e-06
  6x8  unsaturated one       2.69e-06 / 2.22e-05     2.85e-05 / 0.000228     6.43e-06 / 5.14e-05
  3x4  reference   all       7.73e-08 / 5.38e-07     1.93e-06 / 1.54e-05     4.92e-07 / 3.93e-06
  3x4  reference   interior  5.06e-08 / 4.62e-07     1.4e-06  / 1.12e-05     4.43e-07 / 3.54e-06
  3x4  reference   corner    4.81e-08 / 4.39e-07     1.93e-06 / 1.54e-05     4.92e-07 / 3.93e-06
  3x4  reference   row       9.44e-08 / 7.55e-07     1.54e-06 / 1.23e-05     1.07e-06 / 8.59e-06
  3x4  reference   one       1.76e-07 / 1.66e-06     6.29e-05 / 0.000503     4.32e-06 / 3.45e-05
  3x4  unsaturated all       7.32e-08 / 7.19e-07     8.92e-07 / 7.13e-06     4.54e-07 / 3.63e-06
  3x4  unsaturated interior  6.47e-08 / 6.09e-07     9.63e-07 / 7.71e-06     1.13e-06 / 9.04e-06
  3x4  unsaturated corner    7.54e-08 / 6.51e-07     8.92e-07 / 7.13e-06     4.54e-07 / 3.63e-06
  3x4  unsaturated row       1.1e-07  / 8.82e-07     2.28e-06 / 1.82e-05     2.83e-06 / 2.27e-05
  3x4  unsaturated one       4.03e-07 / 3.22e-06     6.81e-05 / 0.000544     3.2e-06  / 2.56e-05
  8x8  reference   all       1.07e-07 / 8.75e-07     1.27e-06 / 1.02e-05     6.69e-07 / 5.35e-06
  8x8  reference   interior  9.17e-08 / 8.02e-07     1.27e-06 / 1.02e-05     6.69e-07 / 5.35e-06
  8x8  reference   corner    8.53e-08 / 7.18e-07     1.27e-06 / 1.02e-05     6.69e-07 / 5.35e-06
  8x8  reference   row       9.67e-08 / 7.74e-07     1.27e-06 / 1.02e-05     6.69e-07 / 5.35e-06
  8x8  reference   one       1.83e-06 / 1.46e-05     0.000116 / 0.000927     3.33e-06 / 2.67e-05
  8x8  unsaturated all       1.42e-07 / 1.13e-06     9.19e-07 / 7.36e-06     2.31e-07 / 1.85e-06
  8x8  unsaturated interior  1.29e-07 / 1.03e-06     9.19e-07 / 7.36e-06     2.31e-07 / 1.85e-06
  8x8  unsaturated corner    1.49e-07 / 1.19e-06     9.19e-07 / 7.36e-06     2.31e-07 / 1.85e-06
  8x8  unsaturated row       1.6e-07  / 1.28e-06     9.19e-07 / 7.36e-06     2.43e-07 / 1.94e-06
  8x8  unsaturated one       5.88e-06 / 4.71e-05     8.3e-05  / 0.000664     6.52e-06 / 5.22e-05
"""
import functools

import numpy as np
import torch

import crf_loss_ref as L
import crf_map_ref as M
import crf_pair_grad_ref as G

F = np.float32
FLT_MIN = L.FLT_MIN
HALF_LOG_PI = 0.5 * np.log(np.pi)
GRIDS = L.GRIDS
BATCHES = [1, 5, 130]
REGIMES = ['reference', 'unsaturated']
MASKS = ['all', 'interior', 'corner', 'row', 'one', 'none']

def mask(rows, cols, name):
    """obs [rows * cols] bool.  'interior': the first superpixel of the pair lists' left side is missing (it has four
    pairs); 'corner': superpixel 0, which no pair touches; 'row': all of row 1; 'one': only the last left-side superpixel
    is observed; 'none': nothing is."""
    left, right = L.pairs(rows, cols)
    nsp = rows * cols
    obs = np.ones(nsp, bool)
    if name == 'interior':
        obs[left[0]] = False
    elif name == 'corner':
        assert 0 not in set(left.tolist()) | set(right.tolist())
        obs[0] = False
    elif name == 'row':
        obs[cols:2 * cols] = False
    elif name == 'one':
        obs[:] = False
        obs[left[-1]] = True
    elif name == 'none':
        obs[:] = False
    else:
        assert name == 'all'
    return obs


def punch(y, obs, fill=np.nan):
    """y with `fill` where obs is False (obs [nsp] for the whole batch, or [B, nsp])."""
    out = np.array(y, F)
    out[~np.broadcast_to(obs, out.shape)] = fill
    return out


# ------------------------------------------------------------------------------------------------ float64
def nll64(z, y, r, left, right):
    """z, y [B, n] (y not finite where there is no target), r [B, npairs] -> dict(mean, per [B], dz [B, n], dr [B, npairs],
    nobs [B], scale [B]) in float64; scale is the loss error's denominator.  LinAlgError / NaN where A is singular."""
    z, r = np.asarray(z, np.float64), np.asarray(r, np.float64)
    y = np.asarray(y, np.float64)
    B, n = z.shape
    left, right = np.asarray(left, np.int64), np.asarray(right, np.int64)
    live = G.owners(left, right)
    per, dz, dr = np.zeros(B), np.zeros((B, n)), np.zeros((B, len(left)))
    nobs, scale = np.zeros(B, np.int64), np.zeros(B)
    for b in range(B):
        O = np.isfinite(y[b])
        m = nobs[b] = int(O.sum())
        if m == 0:
            continue
        A = M.matrix(r[b], n, left, right)
        inv = np.linalg.inv(A)
        C = inv[np.ix_(O, O)]
        mu = inv @ z[b]
        e = y[b, O] - mu[O]
        u = np.linalg.solve(C, e)
        sign, logdet = np.linalg.slogdet(C)
        quad = e @ u
        per[b] = quad + 0.5 * logdet + m * HALF_LOG_PI if sign > 0 else np.nan
        scale[b] = abs(quad) + abs(0.5 * logdet) + m * HALF_LOG_PI
        q = inv[:, O] @ u
        dz[b] = -2 * q / B
        vq, vm = q[left] - q[right], mu[left] - mu[right]
        T = inv[np.ix_(O, left)] - inv[np.ix_(O, right)]              # column k: t of pair k
        tCt = np.einsum('ik,ik->k', T, np.linalg.solve(C, T))
        dr[b] = np.where(live, (2 * vq * vm + vq * vq - 0.5 * tCt) / B, 0.0)
    return dict(mean=per.sum() / B, per=per, dz=dz, dr=dr, nobs=nobs, scale=scale)


def literal_loss(z, y, r, left, right):
    """sum_b L_b / B on torch float64 tensors z [B, n], r [B, npairs] (differentiable) and the array y (NaN = no target):
    A scattered as crf_pair_grad_ref.literal_loss does, C a sub-block of torch.linalg.inv(A)."""
    B, n = z.shape
    li, ri = torch.as_tensor(np.asarray(left, np.int64)), torch.as_tensor(np.asarray(right, np.int64))
    eye = torch.eye(n, dtype=z.dtype)
    total = torch.zeros((), dtype=z.dtype)
    for b in range(B):
        O = torch.as_tensor(np.isfinite(np.asarray(y[b])))
        m = int(O.sum())
        if m == 0:
            continue
        R = torch.zeros((n, n), dtype=z.dtype)
        for q in range(len(li)):
            R = R.index_put((li[q], ri[q]), r[b, q])
            R = R.index_put((ri[q], li[q]), r[b, q])
        A = eye + torch.diag(R.sum(dim=1)) - R
        inv = torch.linalg.inv(A)
        C = inv[O][:, O]
        e = torch.as_tensor(np.asarray(y[b], np.float64))[O] - (inv @ z[b])[O]
        total = total + e @ torch.linalg.solve(C, e) + 0.5 * torch.logdet(C) + m * HALF_LOG_PI
    return total / B


def autograd64(z, y, r, left, right):
    """(loss, dz, dr) of literal_loss by torch autograd in float64."""
    zt = torch.tensor(np.asarray(z, np.float64), requires_grad=True)
    rt = torch.tensor(np.asarray(r, np.float64), requires_grad=True)
    loss = literal_loss(zt, y, rt, left, right)
    if not loss.requires_grad:                                   # nothing observed anywhere
        return 0.0, np.zeros(zt.shape), np.zeros(rt.shape)
    loss.backward()
    return float(loss.detach()), zt.grad.numpy(), rt.grad.numpy()


# ------------------------------------------------------------------------------------------------ float32
def _eliminate32(Um, nn):
    """eliminate of crf.hip on Um [B, nn, cols] float32 in place -> its (logdet [B], positive [B])."""
    B = Um.shape[0]
    idx = np.arange(B)
    ld, ok, swaps = np.zeros(B, F), np.ones(B, bool), np.zeros(B, np.int64)
    for k in range(nn):
        col = np.abs(Um[:, k:, k])
        col = np.where(np.isnan(col), F(np.inf), col)
        arg = k + np.argmax(col, axis=1)                         # the first of equal maxima: the lowest row
        swaps += arg != k
        tmp = Um[idx, k].copy()
        Um[idx, k] = Um[idx, arg]
        Um[idx, arg] = tmp
        piv = Um[:, k, k].copy()
        ok &= (piv > 0) & (piv < np.inf)
        ld = ld + np.log(piv)
        f = Um[:, k + 1:, k] / piv[:, None]
        Um[:, k + 1:, k:] = Um[:, k + 1:, k:] - f[:, :, None] * Um[:, None, k, k:]
    return ld, ok & (swaps % 2 == 0)


def _back32(Um, nn):
    """back_substitute of crf.hip: X [B, nn, cols - nn], column 0 the solution of column nn, the others behind it."""
    X = np.zeros((Um.shape[0], nn, Um.shape[2] - nn), F)
    for i in range(nn - 1, -1, -1):
        s = Um[:, i, nn:].copy()
        for j in range(i + 1, nn):
            s = s - Um[:, i, j, None] * X[:, j]
        X[:, i] = s / Um[:, i, i, None]
    return X


def _s32(inv, a, b):
    return ((inv[:, a, a] + inv[:, b, b]) - inv[:, a, b]) - inv[:, b, a]


def _nll32_group(z, y, r, left, right, obs, inv_b):
    """The images of one batch that share the mask obs [n]; inv_b = fl(1 / B) of the whole batch."""
    Bg, n = z.shape
    live = G.owners(left, right)
    m, km = int(obs.sum()), int((~obs).sum())
    if m == 0:
        return np.zeros(Bg, F), np.zeros((Bg, n), F), np.zeros((Bg, len(left)), F), np.zeros(Bg, np.int32)
    R = np.zeros((Bg, n, n), F)
    for q in range(len(left)):
        R[:, left[q], right[q]] = r[:, q]
        R[:, right[q], left[q]] = r[:, q]
    rs = np.zeros((Bg, n), F)
    for j in range(n):
        rs = rs + R[:, :, j]
    A = -R
    d = np.arange(n)
    A[:, d, d] = (F(1) + rs) - R[:, d, d]
    eye = np.broadcast_to(np.eye(n, dtype=F), (Bg, n, n))
    Um = np.concatenate([A, z[:, :, None], eye], axis=2)
    ld_a, ok_a = _eliminate32(Um, n)
    X = _back32(Um, n)
    mu, inv = X[:, :, 0], X[:, :, 1:]
    s_a = _s32(inv, left, right)
    yh = np.where(obs[None, :], y, F(0)).astype(F)
    mi = np.flatnonzero(~obs)
    rank = np.cumsum(~obs) - 1
    s = np.zeros((Bg, km), F)
    for j in range(n):
        s = s + A[:, mi, j] * yh[:, j:j + 1]
    Um2 = np.concatenate([A[:, mi][:, :, mi], (z[:, mi] - s)[:, :, None],
                          np.broadcast_to(np.eye(km, dtype=F), (Bg, km, km))], axis=2)
    ld_m, ok_m = _eliminate32(Um2, km)
    X2 = _back32(Um2, km)
    xm, minv = X2[:, :, 0], X2[:, :, 1:]
    q = yh.copy()
    q[:, mi] = xm
    q = q - mu
    aq = np.zeros((Bg, n), F)
    for j in range(n):
        aq = aq + A[:, :, j] * q[:, j:j + 1]
    qAq = L._wave_sum(L._pad64(q * aq))
    per = (qAq + F(0.5) * (ld_m - ld_a)) + F(m) * F(HALF_LOG_PI)
    dz = (F(-2) * q) * inv_b
    pad = np.zeros((Bg, n, n), F)                                # A_MM^-1 padded with zeros
    pad[np.ix_(np.arange(Bg), mi, mi)] = minv
    s_m = np.zeros((Bg, len(left)), F)
    for k in range(len(left)):
        a, b = left[k], right[k]
        if not obs[a] and not obs[b]:
            s_m[:, k] = ((pad[:, a, a] + pad[:, b, b]) - pad[:, a, b]) - pad[:, b, a]
        elif not obs[a]:
            s_m[:, k] = pad[:, a, a]
        elif not obs[b]:
            s_m[:, k] = pad[:, b, b]
    vq, vm = q[:, left] - q[:, right], mu[:, left] - mu[:, right]
    dr = (((F(2) * vq) * vm + vq * vq) - F(0.5) * (s_a - s_m)) * inv_b
    dr = np.where(live[None, :], dr, F(0))
    bad = ~(ok_a & ok_m & np.isfinite(per))
    per[bad], dz[bad], dr[bad] = np.nan, np.nan, np.nan
    return per, dz, dr, bad.astype(np.int32)


def nll32(z, y, r, left, right):
    """The kernel's arithmetic in numpy float32 -> dict(mean, per, dz, dr, nobs, status); images that share a mask are
    computed together."""
    z, r = np.ascontiguousarray(z, F), np.ascontiguousarray(r, F)
    y = np.ascontiguousarray(y, F)
    B, n = z.shape
    left, right = np.asarray(left, np.int64), np.asarray(right, np.int64)
    obs = np.isfinite(y)
    per, dz, dr = np.zeros(B, F), np.zeros((B, n), F), np.zeros((B, len(left)), F)
    status = np.zeros(B, np.int32)
    inv_b = F(1) / F(B)
    with np.errstate(all='ignore'):
        for key in {row.tobytes() for row in obs}:
            rows = np.flatnonzero([row.tobytes() == key for row in obs])
            per[rows], dz[rows], dr[rows], status[rows] = _nll32_group(z[rows], y[rows], r[rows], left, right,
                                                                       obs[rows[0]], inv_b)
    return dict(mean=L.mean32(per), per=per, dz=dz, dr=dr, nobs=obs.sum(axis=1).astype(np.int32), status=status)


# ------------------------------------------------------------------------------------------------ errors and bounds
def errors(got, ref):
    """(loss, dz, dr) per-image errors of a float32 result dict (or (per, dz, dr)) against nll64's dict."""
    per, dz, dr = (got['per'], got['dz'], got['dr']) if isinstance(got, dict) else got
    e_loss = np.abs(np.asarray(per, np.float64) - ref['per']) / np.maximum(ref['scale'], FLT_MIN)
    e_dz = G.dr_errors(dz, ref['dz'])                            # the same measure: ||.||inf relative, per image
    e_dr = G.dr_errors(dr, ref['dr']) if dr is not None else np.zeros(len(e_loss))
    return e_loss, e_dz, e_dr


@functools.lru_cache(maxsize=None)
def case(rows, cols, batch, regime, name):
    """(z, y with NaN by the mask, r) of crf_loss_ref.draw, read-only."""
    z, y, r = L.draw(rows, cols, batch, regime)
    y = punch(y, mask(rows, cols, name))
    y.setflags(write=False)
    return z, y, r


@functools.lru_cache(maxsize=None)
def reference(rows, cols, batch, regime, name):
    return nll64(*case(rows, cols, batch, regime, name), *L.pairs(rows, cols))


@functools.lru_cache(maxsize=None)
def restatement(rows, cols, batch, regime, name):
    return nll32(*case(rows, cols, batch, regime, name), *L.pairs(rows, cols))


@functools.lru_cache(maxsize=None)
def measured(rows, cols, regime, name):
    """Worst (loss, dz, dr) error of nll32 against nll64 over BATCHES."""
    worst = np.zeros(3)
    for batch in BATCHES:
        e = errors(restatement(rows, cols, batch, regime, name), reference(rows, cols, batch, regime, name))
        worst = np.maximum(worst, [x.max() for x in e])
    return tuple(float(w) for w in worst)


def bound(rows, cols, regime, name):
    """8 x measured(): (loss, dz, dr)."""
    return tuple(8 * w for w in measured(rows, cols, regime, name))


def positive_definite(rows, cols, batch, regime):
    """Every image's A of the draw is positive definite in float64 (its smallest eigenvalue)."""
    _, _, r = L.draw(rows, cols, batch, regime)
    left, right = L.pairs(rows, cols)
    return min(np.linalg.eigvalsh(M.matrix(r[b], rows * cols, left, right)).min() for b in range(batch)) > 0


# ------------------------------------------------------------------------------------------------ superpixel mean
def superpixel_mean_valid64(x, sp, min_count):
    """x [n, h, w, 1] -> (y [n, P] float64 with NaN below the count, count [n, P]): exact where every sum is."""
    x = np.asarray(x, np.float64)[..., 0]
    n, h, w = x.shape
    blocks = x.reshape(n, h // sp, sp, w // sp, sp).transpose(0, 1, 3, 2, 4).reshape(n, -1, sp * sp)
    fin = np.isfinite(blocks)
    count = fin.sum(axis=2)
    total = np.where(fin, blocks, 0.0).sum(axis=2)
    with np.errstate(all='ignore'):
        y = np.where(count >= max(1, min_count), total / count, np.nan)
    return y, count.astype(np.int32)
