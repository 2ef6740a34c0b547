"""References of a3dp_crf_loss_grad, a3dp_pair_dense_bwd and a3dp_sgd_apply_floor (include/a3d_pairwise.h): the gradient
of the CRF loss of tests/crf_loss_ref.py with respect to the pair weights r, the CRF matrix A = I + D - R no longer a
constant, and the bounds the GPU tests hold the kernel to (tests/test_crf_pair_grad_cpu.py,
tests/test_gpu_crf_pair_grad.py, tests/test_gpu_dcnf_pairwise_train.py).  Pairs, draws, grids, batches, regimes and the
float64 / float32 loss are crf_loss_ref's, unchanged.

grad64     the closed form in float64 on crf_map_ref.matrix.  dA / dr_q = (e_l - e_r)(e_l - e_r)^T for a pair that owns
           its two cells, so with w = A^-1 z, sd = sqrt(det A) and the loss's own fac, ex, Z, u:
             S_q = A^-1[l,l] + A^-1[r,r] - A^-1[l,r] - A^-1[r,l]
             dE_q = (y_l - y_r)^2      dg_q = -(w_l - w_r)^2      dfac_q = -fac / (sd + eps) (sd / 2) S_q
             du_q = u (-dE_q) - (u / Z)(dfac_q ex + fac ex dg_q)        dr[b, q] = -du_q / (u + eps) / B
           A pair whose cells a later pair overwrote is not in A: 0.  -> dr [B, npairs].
autograd64 torch float64 autograd of the literal loss (src/models.py:129-177: scatter, I + D - R, det ** .5, inverse +
           eps), the check of grad64 that does not share its algebra.
grad32     loss32's arithmetic carried over [A | z | I] in numpy float32 in the kernel's order: the same exchanges and row
           operations on 2n + 1 columns, column c of A^-1 back-substituted as the z column is, S_q = ((a_ll + a_rr) - a_lr)
           - a_rl, dfac_q = -((fac / (sd + eps)) (sd 0.5)) S_q.  -> (mean, per_image, dz, det, swaps, dr), the first five
           the bits of loss32.

Bounds.  For every (grid, regime) and the batches 1, 5, 64 and 130 of crf_loss_ref.draw(), the per-image
||dr32 - dr64||inf / ||dr64||inf; the kernel is held to 8 x the worst such figure over the regime's draws, the rule and
the margin of crf_loss_ref's dz bound (the margin tests/test_gpu_crf_map.py leaves for another summation order).
No row needed an absolute bound: where the loss is pinned at -log(eps) ('reference' on 6x8 and 8x8) u is far below eps
and dr, like dz, is small (||dr||inf 1e-5 .. 4e-3 per image) but every term of du scales with u alike, so the relative
error does not grow.  tests/test_crf_pair_grad_cpu.py recomputes the table and pins the constants to it.

  measured (float32 restatement vs float64)     bound = 8 x     kernel on an MI355X reached
  grid  regime        worst dr                  dr              dr
  6x8   reference     5.56e-06                  4.5e-05         not run
  6x8   unsaturated   2.92e-06                  2.4e-05         not run
  6x8   pivoting      0.000241                  0.002           not run
  3x4   reference     6.05e-07                  4.9e-06         not run
  3x4   unsaturated   5.37e-07                  4.3e-06         not run
  3x4   pivoting      3.95e-06                  3.2e-05         not run
  8x8   reference     6.52e-06                  5.3e-05         not run
  8x8   unsaturated   3.43e-06                  2.8e-05         not run
  8x8   pivoting      1.07e-05                  8.6e-05         not run

6x8 'pivoting' is one image of the batch of 64 (cond_inf(A) = 1.4e4, crf_loss_ref's worst too).  ||dr64||inf per image spans
5e-8 (8x8 'reference') .. 66 (6x8 'pivoting').

Descent.  descent_case / descend64: projected gradient descent (lr 0.1, floor 0) on the dense layer alone over a fixed
batch of 5, float64.  From (w, b) = ((1, 1), 1) on 6x8 the loss goes 12.257 -> 12.109 in 12 steps, from ((0.3, 0), 0) on
3x4 6.469 -> 5.308, strictly decreasing both, the weights never at the floor.
"""
import functools

import numpy as np
import torch

import crf_loss_ref as L
import crf_map_ref as M

F = np.float32
FLT_MIN = L.FLT_MIN

# 8 x the measured worst, rounded up to two digits: {(rows, cols): {regime: dr bound}}
BOUNDS = {
    (6, 8): {'reference': 4.5e-05, 'unsaturated': 2.4e-05, 'pivoting': 0.002},
    (3, 4): {'reference': 4.9e-06, 'unsaturated': 4.3e-06, 'pivoting': 3.2e-05},
    (8, 8): {'reference': 5.3e-05, 'unsaturated': 2.8e-05, 'pivoting': 8.6e-05},
}


# edge_case(): four pairs on three nodes, r in 0.25 .. 3, a live loss (0.31 and 1.54): measured 5.54e-06 (its second image)
EDGE_BOUND = 4.5e-05


def edge_case():
    """Pairs (0,1), (1,0), (2,2), (1,2) on three nodes, two images: (1,0) overwrites both cells of (0,1); (2,2) pairs a
    superpixel with itself; (1,2) touches the overwritten pair's node only.  -> (z, y, r, left, right)."""
    z, y = np.array([[0.5, 0.25, 1.0], [0.3, 0.9, 0.2]], F), np.array([[0.5, 0.5, 0.75], [0.25, 1.0, 0.125]], F)
    r = np.array([[0.25, 2.0, 0.5, 1.5], [3.0, 0.5, 0.75, 0.25]], F)
    return z, y, r, [0, 1, 2, 1], [1, 0, 2, 2]


def owners(left, right):
    """live[q]: pair q still owns its two cells after every pair was scattered in order."""
    last = {}
    for q in range(len(left)):
        last[frozenset((int(left[q]), int(right[q])))] = q
    return np.array([last[frozenset((int(left[q]), int(right[q])))] == q for q in range(len(left))])


# ------------------------------------------------------------------------------------------------ float64
def grad64(z, y, r, left, right, eps=L.EPSILON):
    """z, y [B, n], r [B, npairs] (float32 values are widened) -> dr [B, npairs] = d mean loss / d r."""
    z, y, r = (np.asarray(a, np.float64) for a in (z, y, r))
    B, n = z.shape
    left, right = np.asarray(left, np.int64), np.asarray(right, np.int64)
    live = owners(left, right)
    dr = np.zeros((B, len(left)))
    fac0 = np.pi ** (n / 2)
    with np.errstate(all='ignore'):
        for b in range(B):
            A = M.matrix(r[b], n, left, right)
            zb, yb = z[b], y[b]
            energy = yb @ A @ yb - 2 * (zb @ yb) + zb @ zb
            det = np.linalg.det(A)
            try:
                inv = np.linalg.inv(A)
            except np.linalg.LinAlgError:
                inv = np.full((n, n), np.nan)
            w = inv @ zb
            zsum = zb.sum()
            g = zb @ w + eps * zsum * zsum - zb @ zb
            sd = np.sqrt(det)
            fac = fac0 / (sd + eps)
            ex = np.exp(g)
            Z = fac * ex + eps
            u = np.exp(-energy) / Z
            S = inv[left, left] + inv[right, right] - inv[left, right] - inv[right, left]
            dE = (yb[left] - yb[right]) ** 2
            dg = -(w[left] - w[right]) ** 2
            dfac = -fac / (sd + eps) * (sd / 2) * S
            du = u * (-dE) - (u / Z) * (dfac * ex + fac * ex * dg)
            dr[b] = np.where(live, (-du / (u + eps)) / B, 0.0)
    return dr


def literal_loss(z, y, r, left, right, eps=L.EPSILON):
    """The reference's loss_part on torch float64 tensors z, y [B, n], r [B, npairs] -> mean loss (differentiable)."""
    B, n = z.shape
    li, ri = torch.as_tensor(np.asarray(left, np.int64)), torch.as_tensor(np.asarray(right, np.int64))
    eye = torch.eye(n, dtype=z.dtype)
    losses = []
    for b in range(B):
        R = torch.zeros((n, n), dtype=z.dtype)
        for q in range(len(li)):                     # both cells in pair order, as crf_map_ref.matrix and the kernels do;
            R = R.index_put((li[q], ri[q]), r[b, q])       # the reference's two scatter_nd_update passes give the same R
            R = R.index_put((ri[q], li[q]), r[b, q])       # whenever no cell is written twice (the model's pair lists)
        A = eye + torch.diag(R.sum(dim=1)) - R
        zb, yb = z[b], y[b]
        energy = yb @ A @ yb - 2 * (zb @ yb) + zb @ zb
        fac = np.pi ** (n / 2) / (torch.linalg.det(A) ** .5 + eps)
        ex = torch.exp(zb @ (torch.linalg.inv(A) + eps) @ zb - zb @ zb)
        Z = fac * ex + eps
        losses.append(-torch.log(torch.exp(-energy) / Z + eps))
    return torch.stack(losses).mean()


def autograd64(z, y, r, left, right, eps=L.EPSILON):
    zt, yt = (torch.tensor(np.asarray(a, np.float64)) for a in (z, y))
    rt = torch.tensor(np.asarray(r, np.float64), requires_grad=True)
    literal_loss(zt, yt, rt, left, right, eps).backward()
    return rt.grad.numpy()


# ------------------------------------------------------------------------------------------------ float32
def grad32(z, y, r, left, right, eps=L.EPSILON):
    """The kernel's arithmetic in numpy float32, all images at once -> (mean, per_image, dz, det, swaps, dr)."""
    z, y, r = (np.ascontiguousarray(a, F) for a in (z, y, r))
    B, n = z.shape
    left, right = np.asarray(left, np.int64), np.asarray(right, np.int64)
    live = owners(left, right)
    eps, idx = F(eps), np.arange(B)
    with np.errstate(all='ignore'):
        R = np.zeros((B, n, n), F)
        for q in range(len(left)):
            R[:, left[q], right[q]] = r[:, q]
            R[:, right[q], left[q]] = r[:, q]
        rs = np.zeros((B, n), F)
        for j in range(n):
            rs = rs + R[:, :, j]
        A = -R
        d = np.arange(n)
        A[:, d, d] = (F(1) + rs) - R[:, d, d]
        ay = np.zeros((B, n), F)
        for j in range(n):
            ay = ay + A[:, :, j] * y[:, j:j + 1]
        yAy, zy, zz, zsum = (L._wave_sum(L._pad64(v)) for v in (y * ay, z * y, z * z, z))
        energy = (yAy - F(2) * zy) + zz
        Um = np.concatenate([A, z[:, :, None], np.broadcast_to(np.eye(n, dtype=F), (B, n, n))], axis=2)     # [A | z | I]
        det, swaps = np.ones(B, F), np.zeros(B, np.int64)
        for k in range(n):
            arg = k + np.argmax(np.abs(Um[:, k:, k]), axis=1)
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
        X = np.zeros((B, n, n + 1), F)                           # column 0: w = A^-1 z; column 1 + c: column c of A^-1
        for i in range(n - 1, -1, -1):
            s = Um[:, i, n:].copy()
            for j in range(i + 1, n):
                s = s - Um[:, i, j, None] * X[:, j]
            X[:, i] = s / Um[:, i, i, None]
        w, inv = X[:, :, 0], X[:, :, 1:]
        zw = L._wave_sum(L._pad64(z * w))
        g = (zw + (eps * zsum) * zsum) - zz
        sd = np.sqrt(det)
        fac = F(np.pi ** (n / 2.0)) / (sd + eps)
        ex = np.exp(g)
        Z = fac * ex + eps
        u = np.exp(-energy) / Z
        per = -np.log(u + eps)
        dE = F(-2) * y + F(2) * z
        dg = (F(2) * w + ((F(2) * eps) * zsum)[:, None]) - F(2) * z
        du = u[:, None] * (-dE) - (u / Z)[:, None] * ((fac * ex)[:, None] * dg)
        inv_b = F(1) / F(B)
        dz = (-du / (u + eps)[:, None]) * inv_b
        # the pairs
        dy, dw = y[:, left] - y[:, right], w[:, left] - w[:, right]
        S = ((inv[:, left, left] + inv[:, right, right]) - inv[:, left, right]) - inv[:, right, left]
        dfac = (-(fac / (sd + eps) * (sd * F(0.5))))[:, None] * S
        duq = u[:, None] * (-(dy * dy)) - (u / Z)[:, None] * (dfac * ex[:, None] + (fac * ex)[:, None] * (-(dw * dw)))
        dr = (-duq / (u + eps)[:, None]) * inv_b
        dr = np.where(live[None, :], dr, F(0))
        dr[np.isnan(per)] = np.nan                               # a NaN loss: the image's whole row
    return L.mean32(per), per, dz, det, swaps, dr


def dr_errors(dr, dr64):
    """Per image ||dr - dr64||inf / ||dr64||inf; a dr below the float32 normal range may have been flushed to 0."""
    dr = np.asarray(dr, np.float64)
    return np.maximum(np.abs(dr - dr64) - FLT_MIN, 0).max(axis=1) / np.maximum(np.abs(dr64).max(axis=1), FLT_MIN)


@functools.lru_cache(maxsize=None)
def reference(rows, cols, batch, regime):
    """grad64 of crf_loss_ref.draw(): computed once, shared, read-only."""
    out = grad64(*L.draw(rows, cols, batch, regime), *L.pairs(rows, cols))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restatement(rows, cols, batch, regime):
    """grad32 of crf_loss_ref.draw(): computed once, shared, read-only."""
    out = grad32(*L.draw(rows, cols, batch, regime), *L.pairs(rows, cols))
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def measured(rows, cols, regime):
    """Worst per-image dr error of grad32 against grad64 over the regime's draws."""
    return float(max(dr_errors(restatement(rows, cols, batch, regime)[5], reference(rows, cols, batch, regime)).max()
                     for batch in L.BATCHES))


def bound(rows, cols, regime):
    return BOUNDS[(rows, cols)][regime]


# ------------------------------------------------------------------------------------------------ dense layer, descent
def dense_bwd64(sims, dr):
    """sims [n, Q, K], dr [n, Q] -> (dw [K], db) in float64."""
    sims, dr = np.asarray(sims, np.float64), np.asarray(dr, np.float64)
    return np.einsum('bq,bqk->k', dr, sims), dr.sum()


def dense_case(count, k, seed=0):
    """Small integers whose every partial sum is exact in float32 in any order: (sims [1, count, k] in 0 .. 4, dr
    [1, count] in -3 .. 3); |sum| <= 12 * count < 2^24 for every count used."""
    rng = np.random.default_rng(1000 * count + 10 * k + seed)
    return (rng.integers(0, 5, (1, count, k)).astype(F), rng.integers(-3, 4, (1, count)).astype(F))


def sgd_floor32(var, g, lr, floor):
    """a3dp_sgd_apply_floor bit for bit: fl(var - fl(lr * g)), then the floor by a comparison a NaN fails."""
    with np.errstate(all='ignore'):
        v = np.asarray(var, F) - F(lr) * np.asarray(g, F)
    return np.where(v < F(floor), F(floor), v).astype(F)


@functools.lru_cache(maxsize=None)
def descent_case(rows, cols):
    """The fixed batch of the descent tests: z, y of the 'unsaturated' batch of 5 and similarities in (0, 1) drawn for
    it: (z, y, sims [5, npairs, 2]), read-only."""
    z, y, _ = L.draw(rows, cols, 5, 'unsaturated')
    rng = np.random.default_rng(L.seed_of(rows, cols, 5, 'unsaturated') + 7)
    sims = rng.uniform(0.05, 0.95, (5, len(L.pairs(rows, cols)[0]), 2)).astype(F)
    sims.setflags(write=False)
    return z, y, sims


def descend64(z, y, sims, left, right, w, b, steps, lr=0.1, floor=0.0):
    """Projected gradient descent on the pairwise dense layer alone, float64: r = sims w + b, one step per iteration ->
    (losses before each step [steps], [(w, b) after each step])."""
    w, b = np.array(w, np.float64), float(b)
    sims = np.asarray(sims, np.float64)
    losses, path = [], []
    for _ in range(steps):
        r = sims @ w + b
        losses.append(L.loss64(z, y, r, left, right)[0])
        dw, db = dense_bwd64(sims, grad64(z, y, r, left, right))
        w, b = np.maximum(w - lr * dw, floor), max(b - lr * db, floor)
        path.append((w.copy(), b))
    return np.array(losses), path
