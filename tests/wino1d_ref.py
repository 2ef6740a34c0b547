"""Host restatement of the 1-D Winograd F(4,5) route (include/a3d_wino1d.h, csrc/wino1d.hip) in numpy float32, stage by stage as
the library runs it: the three matrices (restated from csrc/wino1d_mats.h as exact fractions and checked against the identity
that defines them), the filter / input / dz transforms, the eight r x 1 products, the output and final transforms, and the two
work-division rules (wino1d_bwd_blocks, wino1d_grad_splits).  Shared by tests/test_wino1d_cpu.py and tests/test_gpu_wino1d.py."""
from fractions import Fraction as F

import numpy as np

POINTS = (F(0), F(1), F(-1), F(2), F(-2), F(1, 2), F(-1, 2))      # and infinity

G = [
    [-1, 0, 0, 0, 0],
    [F(-2, 9), F(-2, 9), F(-2, 9), F(-2, 9), F(-2, 9)],
    [F(-2, 9), F(2, 9), F(-2, 9), F(2, 9), F(-2, 9)],
    [F(1, 90), F(1, 45), F(2, 45), F(4, 45), F(8, 45)],
    [F(1, 90), F(-1, 45), F(2, 45), F(-4, 45), F(8, 45)],
    [F(32, 45), F(16, 45), F(8, 45), F(4, 45), F(2, 45)],
    [F(32, 45), F(-16, 45), F(8, 45), F(-4, 45), F(2, 45)],
    [0, 0, 0, 0, 1],
]
AT = [
    [1, 1, 1, 1, 1, 1, 1, 0],
    [0, 1, -1, 2, -2, F(1, 2), F(-1, 2), 0],
    [0, 1, 1, 4, 4, F(1, 4), F(1, 4), 0],
    [0, 1, -1, 8, -8, F(1, 8), F(-1, 8), 1],
]
BT = [
    [-1, 0, F(21, 4), 0, F(-21, 4), 0, 1, 0],
    [0, 1, 1, F(-17, 4), F(-17, 4), 1, 1, 0],
    [0, -1, 1, F(17, 4), F(-17, 4), -1, 1, 0],
    [0, F(1, 2), F(1, 4), F(-5, 2), F(-5, 4), 2, 1, 0],
    [0, F(-1, 2), F(1, 4), F(5, 2), F(-5, 4), -2, 1, 0],
    [0, 2, 4, F(-5, 2), -5, F(1, 2), 1, 0],
    [0, -2, 4, F(5, 2), -5, F(-1, 2), 1, 0],
    [0, -1, 0, F(21, 4), 0, F(-21, 4), 0, 1],
]


def as_array(m, dtype):
    return np.array([[float(F(v)) for v in row] for row in m], dtype=dtype)


G32, AT32, BT32 = (as_array(m, np.float32) for m in (G, AT, BT))      # float(Fraction) rounds correctly, and so does float32(double) here
G64 = as_array(G, np.float64)      # the filter gradient's final transform runs in double (kW1Gd)

PLANES, BLOCK_SLOTS, CUS = 8, 512, 256
MIN_SHARE, MIN_KTILES = 4, 5

# (n, h, w, c, k, r, padding, ldx, ldy): widths that end a tile at 1, 2, 3 and 4 valid columns (5, 6, 7, 8) and 37; a 5-high
# window over h = 3 (the vertical halo is larger than the image); h = 27; the channel pairs (8, 12), (96, 256) and (6, 5), the
# last in the scalar form; pixel strides wider than the channel counts; a 3-high window; one split and uneven ones; and 100 input
# channels, more than the 96 columns of bwd-data's narrow product tile: the 128 x 128 one, two stream-K blocks a plane.
CASES = [
    (1, 3, 5, 8, 12, 5, 'SAME', None, None),
    (2, 3, 6, 8, 12, 5, 'SAME', 12, 16),
    (3, 6, 7, 6, 5, 5, 'SAME', None, None),
    (2, 7, 8, 8, 12, 5, 'VALID', None, None),
    (1, 9, 9, 6, 5, 5, 'VALID', 7, 9),
    (2, 5, 9, 8, 12, 3, 'SAME', None, None),
    (2, 27, 37, 8, 12, 5, 'SAME', None, None),
    (1, 27, 37, 96, 256, 5, 'SAME', None, None),
    (3, 27, 37, 96, 256, 5, 'SAME', None, None),
    (2, 6, 9, 100, 64, 5, 'SAME', None, None),
]


def case_id(case):
    return 'x'.join(str(v) for v in case[:7])


def geometry(h, w, r, padding):
    """ho, wo, pad_t, pad_l of a stride-1 convolution with an r x 5 window"""
    if padding == 'SAME':
        return h, w, (r - 1) // 2, 2
    return h - r + 1, w - 4, 0, 0


def pad4(c):
    return (c + 3) // 4 * 4


def identity_error():
    """max over (i, k, l) of | sum_j A^T[i][j] G[j][k] B^T[j][l] - [l == i + k] | in float64"""
    a, g, b = (as_array(m, np.float64) for m in (AT, G, BT))
    want = np.zeros((4, 5, 8))
    for i in range(4):
        for k in range(5):
            want[i, k, i + k] = 1.0
    return float(np.abs(np.einsum('ij,jk,jl->ikl', a, g, b) - want).max())


def defining_forms_hold():
    """A^T[i][j] = a_j^i, G[j][k] = a_j^k / prod_{l != j} (a_j - a_l), the rows / columns of the point at infinity: exactly"""
    for j, a in enumerate(POINTS):
        f = F(1)
        for l, b in enumerate(POINTS):
            if l != j:
                f *= a - b
        if [F(AT[i][j]) for i in range(4)] != [a ** i for i in range(4)] or [F(G[j][k]) for k in range(5)] != [a ** k / f for k in range(5)]:
            return False
    return [AT[i][7] for i in range(4)] == [0, 0, 0, 1] and list(G[7]) == [0, 0, 0, 0, 1]


def apply(m, v):
    """out[j] = sum_l m[j][l] v[l] in v's type, ascending l, zero entries skipped (w1_apply)"""
    out = []
    for row in m:
        acc = np.zeros_like(v[0])
        for c, t in zip(row, v):
            if c != 0:
                acc = acc + c * t
        out.append(acc)
    return np.stack(out)


def windows(src, off, tw, width):
    """src [n][H][W][C] -> [width][n][H][tw][C]: column b of the window at column 4 t - off, zeros outside the row"""
    n, hh, ww, c = src.shape
    lo, hi = off, max(0, 4 * (tw - 1) - off + width - ww)
    p = np.pad(src, ((0, 0), (0, 0), (lo, hi), (0, 0)))
    return np.stack([p[:, :, b:b + 4 * (tw - 1) + 1:4, :] for b in range(width)])


def bwd_blocks(tiles, nk):
    return max(1, min(BLOCK_SLOTS // PLANES, tiles * nk // MIN_SHARE))


def grad_splits(m, n, pixels):
    blocks1 = PLANES * -(-m // 128) * -(-n // 128)
    nk = -(-pixels // 32)
    smax = max(1, min(BLOCK_SLOTS // blocks1, nk // MIN_KTILES))
    s, load = 1, -(-blocks1 // CUS)
    for t in range(2, smax + 1):
        l = -(-blocks1 * t // CUS)
        if l * s <= load * t:      # the larger count on a tie
            s, load = t, l
    per = -(-nk // s)
    return -(-nk // per)


def ktile_shares(pixels, splits):
    nk = -(-pixels // 32)
    per = -(-nk // splits)
    return [min(per, nk - z * per) for z in range(splits)]


def bwd_data_geometry(n, h, w, c, k, r, padding):
    ho, wo, _, _ = geometry(h, w, r, padding)
    tw = -(-w // 4)
    kp, np_ = pad4(k), pad4(c)
    bn = 96 if np_ <= 96 else 128
    tiles = -(-n * h * tw // 128) * -(-np_ // bn)
    nk = -(-r * kp // 32)
    return dict(tw=tw, pv=n * ho * tw, pm=n * h * tw, kp=kp, np=np_, bn=bn, tiles=tiles, nk=nk, blocks=bwd_blocks(tiles, nk))


def up(b):
    return (b + 255) // 256 * 256


def bwd_data_ws_bytes(n, h, w, c, k, r, padding, prepared=False):
    g = bwd_data_geometry(n, h, w, c, k, r, padding)
    u = 0 if prepared else up(PLANES * r * g['kp'] * g['np'] * 4)
    return u + up(PLANES * g['pv'] * g['kp'] * 4) + up(PLANES * g['pm'] * g['np'] * 4) + up(PLANES * 2 * g['blocks'] * 128 * g['bn'] * 4)


def prepared_bytes(c, k, r):
    return up(PLANES * r * pad4(k) * pad4(c) * 4)


def bwd_filter_ws_bytes(n, h, w, c, k, r, padding):
    ho, wo, _, _ = geometry(h, w, r, padding)
    tw = -(-wo // 4)
    cp, kp = pad4(c), pad4(k)
    s = grad_splits(r * cp, kp, n * ho * tw)
    return up(PLANES * n * h * tw * cp * 4) + up(PLANES * n * ho * tw * kp * 4) + up(PLANES * s * r * cp * kp * 4) + up(s * kp * 4)


def bwd_data(dz, w, xshape, padding, mask=None):
    """dx [n][h][w][c] from dz [n][ho][wo][k] and w [r][5][c][k], float32 throughout"""
    n, h, wd, c = xshape
    r = w.shape[0]
    k = w.shape[3]
    _, _, pad_t, pad_l = geometry(h, wd, r, padding)
    tw = -(-wd // 4)
    # 1. U[xi][r][k][c] = sum_s G[xi][s] w[r-1-r'][4-s][c][k]
    flipped = w[::-1, ::-1].transpose(1, 0, 3, 2)                       # [s][r][k][c]
    U = apply(G32, flipped)                                             # [8][r][k][c]
    # 2. V[xi][n][ho][tw][k] = B^T of the windows at column 4 t - (4 - pad_l)
    V = apply(BT32, windows(dz, 4 - pad_l, tw, 8))
    # 3. M[xi][n][i][t][c] = sum_r V[xi][n][i - (r - 1 - pad_t) + r'][t][.] U[xi][r'], rows outside dz zero
    top = r - 1 - pad_t
    ho = dz.shape[1]
    Vp = np.pad(V, ((0, 0), (0, 0), (top, max(0, h - 1 - top + r - ho)), (0, 0), (0, 0)))
    M = np.zeros((PLANES, n, h, tw, c), np.float32)
    for xi in range(PLANES):
        cols = np.concatenate([Vp[xi][:, rr:rr + h] for rr in range(r)], axis=-1)      # [n][h][tw][r k]
        M[xi] = (cols.reshape(-1, r * k) @ U[xi].reshape(r * k, c)).reshape(n, h, tw, c)
    # 4. dx = A^T M, columns >= w dropped
    Y = apply(AT32, M)                                                  # [4][n][h][tw][c]
    dx = Y.transpose(1, 2, 3, 0, 4).reshape(n, h, 4 * tw, c)[:, :, :wd]
    if mask is not None:
        dx = np.where(mask > 0, dx, np.float32(0))
    assert dx.dtype == np.float32
    return dx


def bwd_filter(x, dz, r, padding):
    """dw [r][5][c][k] and db [k] from x [n][h][w][c] and dz [n][ho][wo][k]: float32 up to the raw sums of the splits (the pixel axis
    split by the rule), their addition and the final transform in double, as wino1d_dw_kernel runs them"""
    n, h, wd, c = x.shape
    _, ho, wo, k = dz.shape
    _, _, pad_t, pad_l = geometry(h, wd, r, padding)
    tw = -(-wo // 4)
    V = apply(BT32, windows(x, pad_l, tw, 8))                           # [8][n][h][tw][c]
    Z = apply(AT32.T, windows(dz, 0, tw, 4))                            # [8][n][ho][tw][k]
    Vp = np.pad(V, ((0, 0), (0, 0), (pad_t, max(0, ho - 1 - pad_t + r - h)), (0, 0), (0, 0)))
    pixels = n * ho * tw
    splits = grad_splits(r * pad4(c), pad4(k), pixels)
    shares = ktile_shares(pixels, splits)
    Msum = np.zeros((PLANES, r * c, k), np.float64)                     # the splits are added, and G^T applied, in double
    bias = None
    for xi in range(PLANES):
        cols = np.concatenate([Vp[xi][:, rr:rr + ho] for rr in range(r)], axis=-1).reshape(pixels, r * c)
        zz = Z[xi].reshape(pixels, k)
        at = 0
        for z, share in enumerate(shares):
            rows = slice(at, min(pixels, at + 32 * share))
            at += 32 * share
            part = cols[rows].T @ zz[rows]
            assert part.dtype == np.float32
            Msum[xi] = part if z == 0 else Msum[xi] + part
            if xi == 1:                                                 # the plane of point 1: a tile's four dz added
                b = zz[rows].sum(axis=0, dtype=np.float32)
                bias = b if z == 0 else bias + b
    dw = apply(G64.T, Msum.reshape(PLANES, r, c, k)).astype(np.float32)  # [5][r][c][k]
    dw = dw.transpose(1, 0, 2, 3)
    assert bias.dtype == np.float32
    return np.ascontiguousarray(dw), bias


def operands(case, seed):
    """x, dz, w and a ReLU mask (about half zeros, laid out as x) of a case.  The three operands are dense normal values: an
    exact zero operand can leave an output element with no non-zero product at all, so that its scale |a| * |b| vanishes, while
    the transforms still carry the rounding of the window's other columns into it; against such an element no relative bound holds
    for any Winograd form (the step test runs the route on real ReLU maps under the rel-L2 bound)."""
    n, h, w, c, k, r, padding = case[:7]
    ho, wo, _, _ = geometry(h, w, r, padding)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h, w, c)).astype(np.float32)
    dz = rng.standard_normal((n, ho, wo, k)).astype(np.float32)
    wt = (rng.standard_normal((r, 5, c, k)) / np.sqrt(5 * r * c)).astype(np.float32)
    mask = np.maximum(rng.standard_normal((n, h, w, c)), 0).astype(np.float32)
    return x, dz, wt, mask
