"""Host restatement of csrc/wino.hip: Winograd F(2x2,3x3) in numpy float32, stage by stage (filter transform, input transform,
sixteen products, output transform), for the forward and for bwd-data (padding 2 - pad, taps flipped, channels swapped); the
cases tests/test_gpu_wino.py runs; and the headroom bound under which ternary operands give exact results."""
import numpy as np

from oracle import tf13_ops as T

# (n, h, w, c, k, padding, ldx, ldy); None: densely packed
CASES = [
    (3, 13, 18, 256, 384, 'SAME', None, None),      # conv2d_2: an M tail of two 128-row tiles, three N tiles
    (3, 13, 18, 384, 256, 'SAME', None, None),
    (1, 9, 9, 5, 7, 'SAME', None, None),            # scalar channel path, odd extents
    (2, 6, 8, 32, 200, 'VALID', None, None),        # pad 0 (bwd-data: pad 2), an N tail of 72
    (1, 1, 1, 4, 4, 'SAME', None, None),            # tiles that are mostly padding
    (1, 2, 3, 8, 8, 'SAME', None, None),
    (3, 13, 18, 32, 200, 'SAME', 40, 208),          # guard columns in x / dx and y / dz
]

F32 = np.float32


def geometry(h, w, padding):
    ho, pt, _ = T.conv_out_size(h, 3, 1, padding)
    wo, pl, _ = T.conv_out_size(w, 3, 1, padding)
    return ho, wo, pt, pl


def filter_transform(g):
    """g [3][3][C][K] float32 -> U [4][4][C][K] = G g G^T, in the kernel's order of operations"""
    g = g.astype(F32)
    a = g[0] + g[2]
    t = np.stack([g[0], (a + g[1]) * F32(0.5), (a - g[1]) * F32(0.5), g[2]])            # [4][3][C][K]
    a = t[:, 0] + t[:, 2]
    return np.stack([t[:, 0], (a + t[:, 1]) * F32(0.5), (a - t[:, 1]) * F32(0.5), t[:, 2]], axis=1)


def input_transform(x, pad_t, pad_l, th, tw):
    """x [n][h][w][C] -> V [4][4][n*th*tw][C] = B^T d B of the 4x4 windows at (2i - pad_t, 2j - pad_l), zeros outside"""
    n, h, w, c = x.shape
    xp = np.zeros((n, 2 * th + 2 + 2, 2 * tw + 2 + 2, c), F32)         # origin (-2, -2): pad <= 2
    hh, ww = min(h, xp.shape[1] - 2), min(w, xp.shape[2] - 2)
    xp[:, 2:2 + hh, 2:2 + ww] = x[:, :hh, :ww]
    d = np.empty((4, 4, n, th, tw, c), F32)
    for a in range(4):
        for b in range(4):
            y0, x0 = 2 - pad_t + a, 2 - pad_l + b
            d[a, b] = xp[:, y0:y0 + 2 * th:2, x0:x0 + 2 * tw:2]
    r = np.stack([d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]])
    v = np.stack([r[:, 0] - r[:, 2], r[:, 1] + r[:, 2], r[:, 2] - r[:, 1], r[:, 1] - r[:, 3]], axis=1)
    return v.reshape(4, 4, n * th * tw, c)


def output_transform(m, n, th, tw, oh, ow):
    """M [4][4][T][N] -> y [n][oh][ow][N] = A^T M A, tile rows / columns beyond oh / ow dropped"""
    r = np.stack([(m[0] + m[1]) + m[2], (m[1] - m[2]) - m[3]])
    y = np.stack([(r[:, 0] + r[:, 1]) + r[:, 2], (r[:, 1] - r[:, 2]) - r[:, 3]], axis=1)      # [2][2][T][N]
    y = y.reshape(2, 2, n, th, tw, -1).transpose(2, 3, 0, 4, 1, 5).reshape(n, 2 * th, 2 * tw, -1)
    return y[:, :oh, :ow]


def conv(src, g, pad_t, pad_l, oh, ow, stats=None):
    """correlation of src with the taps g [3][3][C][N] at origin -pad, through the four stages in float32"""
    n = src.shape[0]
    th, tw = (oh + 1) // 2, (ow + 1) // 2
    u = filter_transform(g)
    v = input_transform(src.astype(F32), pad_t, pad_l, th, tw)
    m = np.matmul(v, u)                                                                     # float32: [4][4][T][N]
    if stats is not None:
        stats.update(max_v=float(np.abs(v).max()), max_u=float(np.abs(u).max()), channels=src.shape[-1])
    return output_transform(m, n, th, tw, oh, ow)


def fwd(x, w, padding, stats=None):
    ho, wo, pt, pl = geometry(x.shape[1], x.shape[2], padding)
    return conv(x, w, pt, pl, ho, wo, stats)


def bwd_data(dz, w, xshape, padding, stats=None):
    _, h, wd, _ = xshape
    _, _, pt, pl = geometry(h, wd, padding)
    return conv(dz, w[::-1, ::-1].transpose(0, 1, 3, 2), 2 - pt, 2 - pl, h, wd, stats)


def headroom(stats):
    """Every value of the pipeline is a multiple of 1/4 when the operands are integers (U: multiples of 1/4); a product sums
    `channels` terms of at most max_v * max_u and an output nine products, so in units of 1/4 nothing exceeds this."""
    return 36 * stats['channels'] * stats['max_v'] * stats['max_u']


def ternary(rng, shape):
    return rng.integers(-1, 2, size=shape).astype(F32)
