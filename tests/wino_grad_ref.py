"""Host restatement of the filter-gradient route of csrc/wino.hip (include/a3d_wino_grad.h) in numpy float32, stage by stage:
V = B^T d B (tests/wino_ref.py's input transform), Z = A dY A^T of each 2x2 tile of dz, the sixteen products over the tile axis
in `splits` pieces added in ascending order, the final transform G^T M G, and db from plane (1,1) of Z; the split rule of
wino_grad_splits; and the headroom bound under which ternary operands give exact results."""
import numpy as np

import wino_ref as W

F32 = np.float32
BM = BN = 128            # the products' tile
BK = 32
BLOCK_SLOTS = 512        # blocks of eight waves the chip holds at once: two on each of its CUs
CUS = 256
MIN_KTILES = 5


def splits(c, k, tiles):
    """wino_grad_splits(c, k, T), a pure function of the three: within one round of the block slots and at least MIN_KTILES
    k-tiles a split on average, the count with the least work on the busiest CU (ceil(blocks / CUS) blocks of 1 / s of a K loop),
    the smaller count on a tie; then no split is left empty"""
    blocks1 = 16 * -(-c // BM) * -(-k // BN)
    nk = -(-tiles // BK)
    smax = max(1, min(BLOCK_SLOTS // blocks1, nk // MIN_KTILES))
    s = min(range(1, smax + 1), key=lambda t: (-(-blocks1 * t // CUS) / t, t))
    per = -(-nk // s)
    return -(-nk // per)


def ktile_shares(tiles, s):
    """k-tiles of each split as the launch deals them"""
    nk = -(-tiles // BK)
    per = -(-nk // s)
    return [min(per, nk - i * per) for i in range(s)]


def dz_transform(dz, th, tw):
    """dz [n][ho][wo][K] -> Z [4][4][n*th*tw][K] = A dY A^T of the 2x2 tiles, zeros beyond ho / wo"""
    n, ho, wo, k = dz.shape
    p = np.zeros((n, 2 * th, 2 * tw, k), F32)
    p[:, :ho, :wo] = dz
    y = [[p[:, a::2, b::2] for b in range(2)] for a in range(2)]
    r = [[y[0][0], y[0][1]], [y[0][0] + y[1][0], y[0][1] + y[1][1]], [y[0][0] - y[1][0], y[0][1] - y[1][1]], [-y[1][0], -y[1][1]]]
    z = np.stack([np.stack([ra[0], ra[0] + ra[1], ra[0] - ra[1], -ra[1]]) for ra in r])
    return z.reshape(4, 4, n * th * tw, k)


def final_transform(m):
    """M [4][4][C][K] -> dw [3][3][C][K] = G^T M G, in the kernel's order of operations"""
    half = F32(0.5)
    hs = (m[1] + m[2]) * half
    t = np.stack([m[0] + hs, (m[1] - m[2]) * half, hs + m[3]])            # [3][4][C][K]
    hs = (t[:, 1] + t[:, 2]) * half
    return np.stack([t[:, 0] + hs, (t[:, 1] - t[:, 2]) * half, hs + t[:, 3]], axis=1)


def bwd_filter(x, dz, padding, stats=None):
    """(dw [3][3][C][K], db [K]) of a stride-1 3x3 layer through the route, in float32"""
    n, h, w, c = x.shape
    k = dz.shape[-1]
    ho, wo, pt, pl = W.geometry(h, w, padding)
    th, tw = (ho + 1) // 2, (wo + 1) // 2
    tiles = n * th * tw
    v = W.input_transform(x.astype(F32), pt, pl, th, tw)                 # [4][4][T][C]
    z = dz_transform(dz.astype(F32), th, tw)                             # [4][4][T][K]
    s = splits(c, k, tiles)
    m, db, t0 = None, None, 0
    for kt in ktile_shares(tiles, s):
        t1 = min(tiles, t0 + kt * BK)
        part = np.matmul(v[:, :, t0:t1].transpose(0, 1, 3, 2), z[:, :, t0:t1])      # float32: [4][4][C][K]
        bpart = z[1, 1, t0:t1].sum(axis=0, dtype=F32)
        m = part if m is None else m + part
        db = bpart if db is None else db + bpart
        t0 = t1
    if stats is not None:
        stats.update(max_v=float(np.abs(v).max()), max_z=float(np.abs(z).max()), tiles=tiles, splits=s)
    return final_transform(m), db


def headroom(stats):
    """Integer operands: V and Z are integers, a product sums `tiles` terms of at most max_v * max_z, and G^T . G turns sixteen
    of them into quarter-integers: below 2^22 every value of the route, in units of 1/4, is an integer below 2^24."""
    return 16 * stats['tiles'] * stats['max_v'] * stats['max_z']
