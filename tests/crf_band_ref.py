"""References of a3db_crf_band_nll and a3db_crf_band_map (include/a3d_crf_band.h) and the bounds their GPU tests hold the
kernel to (tests/test_crf_band_cpu.py, tests/test_gpu_crf_band.py, tests/test_gpu_dcnf_superpixel.py).

The field is y ~ N(mu, A^-1 / 2), mu = A^-1 z, A = I + D - R from the pair weights; every superpixel is observed:
    L = e^T A e - 1/2 log det A + (n / 2) log pi,   e = y - mu,   the batch objective sum_b L_b / B
    dL/dz = -2 e,   dL/dr_k = 2 (e_l - e_r)(mu_l - mu_r) + (e_l - e_r)^2 - 1/2 S_k(A^-1),  S_k(X) = X_ll + X_rr - 2 X_lr.
Scatter: the pairs in order, the last writer owns a cell {l, r}; an overwritten pair and a pair of a superpixel with itself
have no part in A and dr = 0.

nll64        the definition in float64 on the dense A: numpy.linalg inv and slogdet.
literal_loss the same definition on torch float64 tensors for autograd, which shares none of the closed forms.
nll32        the kernel's own arithmetic in numpy float32 (no FMA), in its order: the band storage S[c][d] = A[c + d][c]
             scattered directly, the diagonal 1 - (sum of the stored -r, columns ascending), right-looking L D L^T with the
             forward solve in the same steps, the division by the pivots, the log determinant as the 256 threads' strided sums
             and the workgroup's sum, the column sweep of L^T mu = D^-1 u, e^T A e = sum D_i ((L^T e)_i)^2 summed the same way, the
             Takahashi recurrence row by row, every entry as eight partial sums added in order, with its 32-lane butterfly for
             the diagonal.  Only logf is numpy's.

Bounds.  The rule of tests/test_gpu_crf_loss.py and tests/test_gpu_crf_observed.py: bound(case) is 8 x the error of nll32
against nll64 on the same inputs (the margin for the device's logf and division); no figure comes from the kernel.  Error
measures, per image: loss |L - L64| / (|e^T A e| + |1/2 log det A| + (n / 2) log pi) (a sum of terms of either sign: the
scale is the size of its terms); dz, dr and mu ||x - x64||inf / ||x64||inf.
Draws: r uniform in [0, 2), z and y uniform in [0.2, 1], seeded by the case: A is strictly diagonally dominant, hence
positive definite, and positive_definite(case) asserts it in float64."""
import functools

import numpy as np
import torch

import crf_loss_ref as L

F = np.float32
FLT_MIN = L.FLT_MIN
HALF_LOG_PI = 0.5 * np.log(np.pi)
THREADS = 256                                 # kThreads of crf_band.hip
GROUPS = THREADS // 32                        # the recurrence's partial sums per entry

GRIDS = {'3x4': (3, 4, 3), '6x8': (6, 8, 3), '5x13': (5, 13, 3), '12x16': (12, 16, 3), '3x32': (3, 32, 3),
         '24x32': (24, 32, 2), '8x8': (8, 8, 3)}
CHAINS = {'chain1': (7, 1, 3), 'chain32': (40, 32, 3)}          # n, the pairs' distance, batch
CASES = list(GRIDS) + list(CHAINS)


def pairs(case):
    """-> (left, right int64 arrays, nsp, band)."""
    if case in GRIDS:
        rows, cols, _ = GRIDS[case]
        left, right = L.pairs(rows, cols)
        return left, right, rows * cols, cols
    n, dist, _ = CHAINS[case]
    left = np.arange(0, n - dist, dtype=np.int64)
    return left, left + dist, n, dist


def batch_of(case):
    return (GRIDS.get(case) or CHAINS[case])[2]


@functools.lru_cache(maxsize=None)
def draw(case):
    """(z, y [B, n], r [B, npairs]) float32, read-only."""
    left, _, n, _ = pairs(case)
    B = batch_of(case)
    rng = np.random.default_rng(7000 + CASES.index(case))
    z, y = (rng.uniform(0.2, 1.0, (B, n)).astype(F) for _ in range(2))
    r = rng.uniform(0.0, 2.0, (B, len(left))).astype(F)
    for a in (z, y, r):
        a.setflags(write=False)
    return z, y, r


def owners(left, right):
    """live[q]: pair q is no self pair and no later pair has its two superpixels."""
    last = {}
    for q in range(len(left)):
        last[(min(left[q], right[q]), max(left[q], right[q]))] = q
    return np.array([left[q] != right[q] and last[(min(left[q], right[q]), max(left[q], right[q]))] == q
                     for q in range(len(left))], bool)


def matrix(r, n, left, right):
    """One image: r [npairs] -> the dense A [n, n] float64."""
    r = np.asarray(r, np.float64)
    R = np.zeros((n, n))
    for q in np.flatnonzero(owners(left, right)):
        R[left[q], right[q]] = R[right[q], left[q]] = r[q]
    return np.eye(n) + np.diag(R.sum(axis=1)) - R


# ------------------------------------------------------------------------------------------------ float64
def nll64(z, y, r, left, right):
    """-> dict(mean, per [B], dz [B, n], dr [B, npairs], mu [B, n], scale [B]) in float64."""
    z, y, r = (np.asarray(a, np.float64) for a in (z, y, r))
    B, n = z.shape
    left, right = np.asarray(left, np.int64), np.asarray(right, np.int64)
    live = owners(left, right)
    per, scale, dz, mu_all = np.zeros(B), np.zeros(B), np.zeros((B, n)), np.zeros((B, n))
    dr = np.zeros((B, len(left)))
    for b in range(B):
        A = matrix(r[b], n, left, right)
        inv = np.linalg.inv(A)
        mu = mu_all[b] = np.linalg.solve(A, z[b])
        e = y[b] - mu
        sign, logdet = np.linalg.slogdet(A)
        quad = e @ A @ e
        per[b] = quad - 0.5 * logdet + n * HALF_LOG_PI if sign > 0 else np.nan
        scale[b] = abs(quad) + abs(0.5 * logdet) + n * HALF_LOG_PI
        dz[b] = -2 * e / B
        ve, vm = e[left] - e[right], mu[left] - mu[right]
        s = inv[left, left] + inv[right, right] - 2 * inv[left, right]
        dr[b] = np.where(live, (2 * ve * vm + ve * ve - 0.5 * s) / B, 0.0)
    return dict(mean=per.sum() / B, per=per, dz=dz, dr=dr, mu=mu_all, scale=scale)


def literal_loss(z, y, r, left, right):
    """sum_b L_b / B on torch float64 tensors z [B, n], r [B, npairs] (differentiable) and the array y."""
    B, n = z.shape
    live = owners(left, right)
    yt = torch.as_tensor(np.asarray(y, np.float64))
    total = torch.zeros((), dtype=z.dtype)
    for b in range(B):
        R = torch.zeros((n, n), dtype=z.dtype)
        for q in np.flatnonzero(live):
            R = R.index_put((torch.tensor([left[q], right[q]]), torch.tensor([right[q], left[q]])), r[b, q])
        A = torch.eye(n, dtype=z.dtype) + torch.diag(R.sum(dim=1)) - R
        e = yt[b] - torch.linalg.solve(A, z[b])
        total = total + e @ A @ e - 0.5 * torch.logdet(A) + n * HALF_LOG_PI
    return total / B


def autograd64(z, y, r, left, right):
    zt = torch.tensor(np.asarray(z, np.float64), requires_grad=True)
    rt = torch.tensor(np.asarray(r, np.float64), requires_grad=True)
    loss = literal_loss(zt, y, rt, left, right)
    loss.backward()
    return float(loss.detach()), zt.grad.numpy(), rt.grad.numpy()


# ------------------------------------------------------------------------------------------------ float32
def _strided_sum(v):
    """band_block_sum of crf_band.hip after the threads' strided sums: v [B, n] -> [B]; thread t adds elements t,
    t + THREADS, ... in order, then the 64-lane butterfly in every wavefront, then the wavefronts in turn."""
    B, n = v.shape
    s = np.zeros((B, THREADS), F)
    for base in range(0, n, THREADS):
        chunk = v[:, base:base + THREADS]
        s[:, :chunk.shape[1]] = s[:, :chunk.shape[1]] + chunk
    total = L._wave_sum(s[:, :64])
    for wave in range(1, THREADS // 64):
        total = total + L._wave_sum(s[:, 64 * wave:64 * wave + 64])
    return total


def nll32(z, y, r, left, right, band):
    """The kernel's arithmetic in numpy float32, all images at once -> dict(mean, per, dz, dr, mu, status)."""
    z, y, r = (np.ascontiguousarray(a, F) for a in (z, y, r))
    B, n = z.shape
    left, right = np.asarray(left, np.int64), np.asarray(right, np.int64)
    live = owners(left, right)
    inv_b = F(1) / F(B)
    with np.errstate(all='ignore'):
        S = np.zeros((B, n, band + 1), F)
        for q in np.flatnonzero(live):
            lo, d = min(left[q], right[q]), abs(left[q] - right[q])
            S[:, lo, d] = F(0) - r[:, q]
        rs = np.zeros((B, n), F)
        for e in range(band, 0, -1):                             # columns i - band .. i - 1
            if e < n:
                rs[:, e:] = rs[:, e:] + S[:, :n - e, e]
        for d in range(1, band + 1):                             # columns i + 1 .. i + band (cells past the end are +0)
            rs = rs + S[:, :, d]
        S[:, :, 0] = F(1) - rs
        zv = z.copy()
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
        ld = _strided_sum(np.log(p))
        zv = zv / p
        S[:, :, 1:] = S[:, :, 1:] / p[:, :, None]
        for k in range(n - 1, 0, -1):
            d = np.arange(1, min(band, k) + 1)
            zv[:, k - d] = zv[:, k - d] - S[:, k - d, d] * zv[:, k:k + 1]
        mu = zv
        ev = y - mu
        s = ev.copy()
        for d in range(1, min(band, n - 1) + 1):
            s[:, :n - d] = s[:, :n - d] + S[:, :n - d, d] * ev[:, d:]
        qf = _strided_sum(S[:, :, 0] * (s * s))
        per = (qf - F(0.5) * ld) + F(n) * F(HALF_LOG_PI)
        dz = (F(-2) * ev) * inv_b
        lanes = np.arange(32)
        for i in range(n - 1, -1, -1):                           # Takahashi, in place
            w = min(band, n - 1 - i)
            col = S[:, i, :].copy()
            prod = np.zeros((B, 32), F)
            if w > 0:
                d = np.arange(1, w + 1)
                part = np.zeros((GROUPS, B, w), F)                # group g: the terms m = 1 + g, 1 + g + GROUPS, ...
                for m in range(1, w + 1):
                    rows = np.where(m <= d, i + m, i + d)
                    g = (m - 1) % GROUPS
                    part[g] = part[g] + col[:, m:m + 1] * S[:, rows, np.abs(d - m)]
                acc = part[0]
                for g in range(1, GROUPS):
                    acc = acc + part[g]
                zij = F(0) - acc
                prod[:, :w] = col[:, 1:w + 1] * zij
                S[:, i, 1:w + 1] = zij
            for off in (16, 8, 4, 2, 1):
                prod = prod + prod[:, lanes ^ off]
            S[:, i, 0] = F(1) / col[:, 0] - prod[:, 0]
        lo, dd = np.minimum(left, right), np.abs(left - right)
        dd = np.where(live, dd, 0)
        zlr = S[:, lo, dd]
        s_a = ((S[:, left, 0] + S[:, right, 0]) - zlr) - zlr
        vq, vm = ev[:, left] - ev[:, right], mu[:, left] - mu[:, right]
        dr = (((F(2) * vq) * vm + vq * vq) - F(0.5) * s_a) * inv_b
        dr = np.where(live[None, :], dr, F(0)).astype(F)
        bad = ~(ok & np.isfinite(per))
        mu = mu.copy()
        per[bad], dz[bad], dr[bad], mu[bad] = np.nan, np.nan, np.nan, np.nan
    return dict(mean=L.mean32(per), per=per, dz=dz, dr=dr, mu=mu, status=bad.astype(np.int32))


# ------------------------------------------------------------------------------------------------ errors and bounds
def _rel_inf(x, x64):
    x = np.asarray(x, np.float64)
    return np.maximum(np.abs(x - x64) - FLT_MIN, 0).max(axis=1) / np.maximum(np.abs(x64).max(axis=1), FLT_MIN)


def errors(got, ref):
    """Per-image (loss, dz, dr, mu) errors of a float32 result dict against nll64's; a missing dr or mu counts as exact."""
    e_loss = np.abs(np.asarray(got['per'], np.float64) - ref['per']) / np.maximum(ref['scale'], FLT_MIN)
    zero = np.zeros(len(e_loss))
    return (e_loss, _rel_inf(got['dz'], ref['dz']), _rel_inf(got['dr'], ref['dr']) if got.get('dr') is not None else zero,
            _rel_inf(got['mu'], ref['mu']) if got.get('mu') is not None else zero)


def bound_of(z, y, r, left, right, band):
    """8 x the restatement's worst error against float64 on these very inputs: (loss, dz, dr, mu)."""
    e = errors(nll32(z, y, r, left, right, band), nll64(z, y, r, left, right))
    return tuple(8 * float(x.max()) for x in e)


@functools.lru_cache(maxsize=None)
def reference(case):
    left, right, _, _ = pairs(case)
    return nll64(*draw(case), left, right)


@functools.lru_cache(maxsize=None)
def restatement(case):
    left, right, _, band = pairs(case)
    return nll32(*draw(case), left, right, band)


@functools.lru_cache(maxsize=None)
def bound(case):
    """8 x the error of nll32 against nll64 on the case's draw: (loss, dz, dr, mu)."""
    return tuple(8 * float(x.max()) for x in errors(restatement(case), reference(case)))


@functools.lru_cache(maxsize=None)
def positive_definite(case):
    left, right, n, _ = pairs(case)
    _, _, r = draw(case)
    return min(np.linalg.eigvalsh(matrix(r[b], n, left, right)).min() for b in range(len(r))) > 0
