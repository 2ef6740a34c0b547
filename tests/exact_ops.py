"""Exact-integer cases for every contraction route: inputs, float64 references, and the conditions that make element-by-
element equality with a float32 / bf16 kernel legitimate.  No GPU and no torch in here (test_exact_cpu.py builds every case
on the CPU; test_gpu_exact.py and exact_forced_worker.py run them).

Why equality needs no tolerance.  Operands are small integers (ternary {-1, 0, 1} unless a case says otherwise) and the
helper asserts, every time it builds a case,
  * every reference value is an integer,
  * K * max|a| * max|b| + max|bias| < 2^24 for the contraction length K of each direction (forward: r s c; bwd-data:
    r s k; bwd-filter: the pixel axis n ho wo).  The bound is on the sum of ABSOLUTE products, so every partial sum of every
    k-tile, split-K slab, stream-K share and reduction order is an integer below 2^24 and therefore exact in float32,
  * an output a kernel stores as bf16 has max|ref| <= 256: bf16 holds every integer up to 256, the rounding is the identity
    and a difference of 1 cannot hide in it.
Operand magnitudes stay <= 256, so bf16 operands and the hi plane of the bf16x3 split are exact (the lo plane is zero).
None of this is measured on a GPU, and no element is ever left out of a comparison."""
import functools

import numpy as np

from oracle import tf13_ops as T

F32_EXACT = 2 ** 24
BF16_EXACT = 256


def ternary(rng, shape):
    return rng.integers(-1, 2, shape).astype(np.float32)


def integers(rng, shape, amax):
    """integers in [-amax, amax] (amax = 1: ternary)"""
    return rng.integers(-amax, amax + 1, shape).astype(np.float32)


def small_bias(rng, k):
    return rng.integers(-3, 4, k).astype(np.float32)


def amax(a):
    return float(np.abs(a).max()) if a.size else 0.0


def require_integers(what, a):
    assert np.array_equal(a, np.rint(a)), f'{what}: the reference is not integer-valued'
    return a


def require_headroom(what, K, a, b, bias=None):
    bound = K * amax(a) * amax(b) + (amax(bias) if bias is not None else 0.0)
    assert bound < F32_EXACT, f'{what}: sum of absolute products may reach {bound} >= 2^24'
    assert amax(a) <= BF16_EXACT and amax(b) <= BF16_EXACT, f'{what}: operands are not exact in bf16'


def require_bf16(what, a):
    """an output stored as bf16: shrink the batch or make the operands sparser if this fails, never loosen it"""
    assert amax(a) <= BF16_EXACT, f'{what}: max|ref| = {amax(a)} > 256, bf16 would round it'
    return a


def f64(a):
    return np.asarray(a, np.float64)


def pool_windows(y):
    """[n, ho, wo, k] -> [n, ho//2, wo//2, k, 4]: the 2x2 windows in (row, column) scan order; an odd last row / column has none"""
    n, ho, wo, k = y.shape
    ph, pw = ho // 2, wo // 2
    return y[:, :2 * ph, :2 * pw].reshape(n, ph, 2, pw, 2, k).transpose(0, 1, 3, 5, 2, 4).reshape(n, ph, pw, k, 4)


def pool_reference(y):
    """(pooled values, uint8 position of the FIRST maximum of each window) — MaxPoolGrad's rule, held bit for bit: the
    activations are integers, so ties are frequent and there is no rounding that could excuse another choice"""
    win = pool_windows(y)
    return win.max(-1), win.argmax(-1).astype(np.uint8)          # numpy argmax = first maximum


def pool_grad_reference(arg, pooled, dy, shape, relu):
    """MaxPoolGrad by recorded position (+ ReluGrad: pooled > 0) -> [n, ho, wo, k]; rows / columns without a window are 0"""
    n, ho, wo, k = shape
    ph, pw = ho // 2, wo // 2
    g = np.where(pooled > 0, dy, 0.0) if relu else dy
    dx = np.zeros(shape, np.float64)
    for pos in range(4):
        dx[:, pos >> 1:2 * ph:2, pos & 1:2 * pw:2, :] = np.where(arg == pos, g, 0.0)
    return dx


class ConvCase:
    """One convolution, all three directions.  y is the pre-activation output WITH the bias; dz multiplies it."""

    def __init__(self, n, h, w, c, k, ks, st, pad, mag=1):
        self.shape = (n, h, w, c, k, ks, st, pad)
        self.what = f'conv {self.shape} |operands| <= {mag}'
        rng = np.random.default_rng(5000 + h * w + c + k)
        self.x = integers(rng, (n, h, w, c), mag)
        self.w = integers(rng, (ks, ks, c, k), mag)
        self.b = small_bias(rng, k)
        self.y = require_integers(self.what + ' y', T.conv2d_fwd(f64(self.x), f64(self.w), f64(self.b), st, pad))
        self.ho, self.wo = self.y.shape[1:3]
        self.dz = integers(rng, self.y.shape, mag)
        dw, db = T.conv2d_bwd_filter(f64(self.x), f64(self.dz), self.w.shape, st, pad)
        self.dw, self.db = require_integers(self.what + ' dw', dw), require_integers(self.what + ' db', db)
        self.dx = require_integers(self.what + ' dx', T.conv2d_bwd_data(f64(self.dz), f64(self.w), self.x.shape, st, pad))
        require_headroom(self.what + ' forward', ks * ks * c, self.x, self.w, self.b)
        require_headroom(self.what + ' bwd-data', ks * ks * k, self.dz, self.w)
        require_headroom(self.what + ' bwd-filter', n * self.ho * self.wo, self.x, self.dz)

    def bf16(self, *names):
        """the named outputs are stored as bf16 somewhere: hold them to 256"""
        for name in names:
            require_bf16(f'{self.what} {name}', getattr(self, name))
        return self

    @functools.cached_property
    def pooled(self):
        """(pooled, argmax) of relu(y)"""
        return pool_reference(np.maximum(self.y, 0))


@functools.lru_cache(maxsize=None)
def conv_case(n, h, w, c, k, ks, st, pad, mag=1):
    return ConvCase(n, h, w, c, k, ks, st, pad, mag)


class BothCase:
    """A one-filter 5x5 stride-1 conv on a buffer of pixel stride ldx >= c (stencil1.hip)"""

    def __init__(self, n, h, w, c, pad, ldx, lddx):
        self.shape = (n, h, w, c, pad, ldx, lddx)
        self.what = f'one-filter conv {self.shape}'
        rng = np.random.default_rng(5700 + n * h * w + c)
        self.xbuf = ternary(rng, (n, h, w, ldx))
        self.x = self.xbuf[..., :c]
        self.w = ternary(rng, (5, 5, c, 1))
        self.b = small_bias(rng, 1)
        self.y = require_integers(self.what + ' y', T.conv2d_fwd(f64(self.x), f64(self.w), f64(self.b), 1, pad))
        self.dz = ternary(rng, self.y.shape)
        dw, db = T.conv2d_bwd_filter(f64(self.x), f64(self.dz), self.w.shape, 1, pad)
        self.dw, self.db = require_integers(self.what + ' dw', dw), require_integers(self.what + ' db', db)
        self.dx = require_integers(self.what + ' dx', T.conv2d_bwd_data(f64(self.dz), f64(self.w), self.x.shape, 1, pad))
        require_headroom(self.what + ' forward', 25 * c, self.x, self.w, self.b)
        require_headroom(self.what + ' bwd-data', 25, self.dz, self.w)
        require_headroom(self.what + ' bwd-filter', n * self.y.shape[1] * self.y.shape[2], self.x, self.dz)
        require_bf16(self.what + ' dx', self.dx)


@functools.lru_cache(maxsize=None)
def both_case(*shape):
    return BothCase(*shape)


class PooledBwdfCase:
    """Filter gradient of conv -> ReLU -> 2x2 max pool from the gradient of the POOLED map (fewch.hip / fewch16.hip): ternary
    `pooled` makes a third of the maxima exactly 0 and a third negative, so ReluGrad's edge `> 0` is held exactly"""

    def __init__(self, n, h, w, c, k, ks, st, ld, lda):
        self.shape = (n, h, w, c, k, ks, st, ld, lda)
        self.what = f'pool-fused filter gradient {self.shape}'
        rng = np.random.default_rng(5900 + h * w + k)
        self.x = ternary(rng, (n, h, w, c))
        self.ho, self.wo = (h - ks) // st + 1, (w - ks) // st + 1
        ph, pw = self.ho // 2, self.wo // 2
        self.pooled = ternary(rng, (n, ph, pw, ld))
        self.dpool = ternary(rng, (n, ph, pw, ld))
        self.arg = rng.integers(0, 4, (n, ph, pw, lda)).astype(np.uint8)
        self.dz = pool_grad_reference(self.arg[..., :k], self.pooled[..., :k], f64(self.dpool[..., :k]), (n, self.ho, self.wo, k), True)
        edge = (self.pooled[..., :k] == 0) & (self.dpool[..., :k] != 0)
        assert edge.mean() > 0.1, 'ReluGrad edge not live'      # maxima of exactly 0 that would pass a gradient on under >=
        dw, db = T.conv2d_bwd_filter(f64(self.x), self.dz, (ks, ks, c, k), st, 'VALID')
        self.dw, self.db = require_integers(self.what + ' dw', dw), require_integers(self.what + ' db', db)
        require_headroom(self.what, n * self.ho * self.wo, self.x, self.dz)


@functools.lru_cache(maxsize=None)
def pooled_bwdf_case(*shape):
    return PooledBwdfCase(*shape)


class DenseCase:
    def __init__(self, m, k, n):
        self.shape = (m, k, n)
        self.what = f'dense {self.shape}'
        rng = np.random.default_rng(5300 + m + k + n)
        self.x = ternary(rng, (m, k))
        self.w = ternary(rng, (k, n))
        self.b = small_bias(rng, n)
        self.keep = rng.random((m, n)) >= 0.5
        self.dz = ternary(rng, (m, n))
        self.y = require_integers(self.what + ' y', f64(self.x) @ f64(self.w) + f64(self.b))
        self.dx = require_integers(self.what + ' dx', f64(self.dz) @ f64(self.w).T)
        self.dw = require_integers(self.what + ' dw', f64(self.x).T @ f64(self.dz))
        self.db = require_integers(self.what + ' db', f64(self.dz).sum(0))
        require_headroom(self.what + ' forward', k, self.x, self.w, 2 * self.b)          # (dropout doubles: still exact)
        require_headroom(self.what + ' bwd-data', 2 * n, self.dz, self.w)                # (scale = 2.0)
        require_headroom(self.what + ' bwd-filter', m, self.x, self.dz)

    def bf16(self):
        """dense_fwd_ex's bf16 second output (relu, dropout x 2) and dense_bwd_data_ex's bf16 dx (scale 2)"""
        require_bf16(self.what + ' 2 y', 2 * self.y)
        require_bf16(self.what + ' 2 dx', 2 * self.dx)
        return self


@functools.lru_cache(maxsize=None)
def dense_case(m, k, n):
    return DenseCase(m, k, n)


# ---- the cases, by route (shapes from tests/test_gpu_ops.py: the smallest known to reach each route) ----
GENERIC = [
    # n, h, w, c, k, ksize, stride, padding
    (2, 27, 37, 96, 256, 5, 1, 'SAME'),      # a k-tile straddles two taps (96 channels), K = 2400: a K tail
    (3, 13, 18, 256, 384, 3, 1, 'SAME'),
    (2, 13, 18, 384, 256, 3, 2, 'VALID'),    # stride 2: bwd-data as one launch per parity class
    (1, 10, 11, 8, 12, 4, 2, 'SAME'),        # asymmetric SAME padding
    (1, 9, 9, 5, 7, 3, 1, 'SAME'),           # scalar operands
    (2, 13, 14, 4, 8, 3, 4, 'VALID'),        # stride 4 > kernel 3: pixels that receive no gradient must be exact zeros
    (1, 1, 1, 16, 8, 1, 1, 'VALID'),
]
# conv2d_1's shape with operands up to 8: sums up to 1.5e5 use 18 bits of the accumulator; float32 kernels only
WIDE = (2, 27, 37, 96, 256, 5, 1, 'SAME', 8)
GUARD = [
    # n, h, w, c, k, ksize, ld: stride 1, SAME, output pitch ld >= k, guard rows behind the tensor
    (2, 21, 30, 64, 64, 5, 64),
    (1, 27, 37, 96, 72, 5, 80),
    (3, 13, 18, 32, 200, 3, 208),
    (1, 9, 11, 16, 4, 3, 12),
]
STRIDED_ONE_LAUNCH = [(20, 31, 33, 64, 48, 3, 2, 'SAME'), (24, 26, 30, 5, 7, 5, 2, 'SAME')]
STRIDED_ONE_LAUNCH_BF16 = [(20, 31, 33, 64, 48, 3, 2, 'SAME'), (3, 9, 10, 8, 8, 1, 2, 'VALID')]     # 1x1: odd classes receive no tap
FEW_CHANNEL = [
    (2, 35, 47, 3, 96, 11, 4, 'VALID'),
    (2, 35, 48, 3, 96, 11, 4, 'VALID'),
    (2, 21, 32, 3, 24, 5, 4, 'VALID'),
    (2, 30, 35, 3, 64, 11, 1, 'VALID'),
    (3, 23, 29, 1, 40, 5, 1, 'VALID'),
    (2, 20, 27, 4, 70, 3, 2, 'VALID'),
    (65, 15, 15, 2, 33, 7, 4, 'VALID'),
    (2, 12, 15, 1, 40, 3, 1, 'VALID'),
    (3, 9, 14, 2, 36, 2, 1, 'VALID'),
    (3, 12, 27, 3, 16, 2, 1, 'SAME'),        # even kernel, SAME: pads on the right / below only
    (4, 25, 38, 1, 2, 2, 1, 'SAME'),
]
POOLED_BWDF = [
    # n, h, w, c, k, ksize, stride, ld, argmax stride
    (2, 35, 48, 3, 96, 11, 4, 96, 96),
    (2, 40, 52, 3, 63, 9, 2, 64, 63),
    (3, 30, 36, 3, 64, 11, 1, 64, 64),
]
BOTH = [
    # n, h, w, c, padding, ldx, lddx
    (2, 21, 30, 64, 'SAME', 64, 64),
    (3, 55, 74, 64, 'SAME', 64, 64),
    (2, 9, 13, 40, 'VALID', 40, 40),
    (5, 7, 6, 64, 'SAME', 64, 72),
    (70, 5, 9, 24, 'SAME', 32, 24),
    (2, 12, 17, 64, 'VALID', 64, 64),
    (1, 19, 70, 64, 'SAME', 64, 64),
]
POOL_FWD = [
    # the cases of test_conv2d_pool_fwd_equals_conv_then_pool at one or two images
    (1, 228, 304, 3, 63, 9, 2, 'VALID'),
    (1, 228, 304, 3, 96, 11, 4, 'VALID'),
    (2, 27, 37, 96, 256, 5, 1, 'SAME'),
    (1, 9, 8, 5, 7, 3, 1, 'SAME'),
    (2, 2, 2, 4, 4, 1, 1, 'VALID'),
    (2, 33, 31, 3, 64, 11, 1, 'VALID'),
    (2, 21, 18, 1, 40, 4, 1, 'VALID'),
]
# 3-channel images stored as 4-channel bf16 pixels: even stride, even width; >= 33 filters: conv3b, fewer: igemm_bf16
POOL_FWD_BF16_IMAGE = [c for c in POOL_FWD if c[3] == 3 and c[6] % 2 == 0] + [(2, 17, 20, 3, 16, 5, 2, 'VALID')]
# bf16 x, w and pooled map: the LDS-DMA kernel's pooling epilogue (k a multiple of 16)
POOL_FWD_BF16_STORED = [(2, 27, 37, 96, 256, 5, 1, 'SAME'), (2, 21, 30, 32, 64, 3, 1, 'VALID')]
BF16_ARITH = [c for c in GENERIC if c[3] % 4 == 0 and c[4] % 4 == 0]
# bf16 tensors of enough tiles for the planner's own pick of the LDS-DMA kernel (forward, bwd-data on the 96-column tile, bwd-filter)
RING = [(26, 27, 37, 96, 128, 5, 1, 'SAME')]
DENSE = [(7, 130, 66), (9, 1024, 1031), (48, 16, 1), (64, 3, 4070), (2, 1, 8), (4, 512, 4070),
         (5, 1028, 1031)]      # the last: m <= 64, k n >= 2^20, rows of x in 16-byte pieces: dense.hip's streaming kernels
DENSE_BF16 = [(9, 1024, 1032), (64, 1024, 1024)]      # bf16 x / dz / dx beside bf16 weights: 64-row tiles of the LDS-DMA kernel


def stores_bf16(case):
    """can the route keep this conv's tensors as bf16 (whole 16-byte pieces of channels)?"""
    return case[3] % 8 == 0 and case[4] % 8 == 0


# ---- pinned tiles, split-K and stream-K (exact_forced_worker.py) ----
NUM_CFGS = 11                        # igemm_cfgs.h: 0-8 register-staged, 9 and 10 LDS-DMA staged (forward only)
TWIN = {9: 7, 10: 8}                 # ... and the register-staged twins that run their other directions
CFG_TILE = {0: (128, 128), 1: (128, 96), 2: (128, 64), 3: (128, 32), 4: (64, 64), 5: (32, 128), 6: (64, 128), 7: (128, 128),
            8: (128, 64), 9: (128, 128), 10: (128, 64)}
FORCED_F32 = [(2, 21, 30, 64, 64, 5, 1, 'SAME'), (3, 13, 18, 32, 200, 3, 1, 'SAME')]      # the second: N tail 72, 9 k-tiles
FORCED_STRIDED = (2, 13, 14, 8, 8, 3, 2, 'VALID')
SPLITS_F32 = (1, 2, 3, 5)
STREAMK_SMALL = (1, 3, 7)
SPLITS_BF16 = (1, 2, 3)
RING_FWD = ((2, 13, 18, 64, 200, 3, 1, 'SAME'), (0, 1, 2, 3, 5, 6))
RING_BWD_D = ((2, 13, 18, 64, 200, 3, 1, 'SAME'), (0, 1, 2, 3, 5, 6))
RING_BWD_D_96 = ((2, 13, 18, 96, 64, 3, 1, 'SAME'), (4,))          # the 96-column tile: bwd-data of 96 input channels
# the filter gradient's GEMM of M = 576 rows over K = 8 * 23 * 23 = 4232 pixels (SAME: the LDS-DMA kernel wants K >= 4096)
RING_BWD_F = ((8, 23, 23, 64, 64, 3, 1, 'SAME'), (0, 1, 2, 3))
MODES = (0, 1, 2)                    # forward, bwd-data, bwd-filter (a3d_timing_record.mode)


def gemm_dims(case, mode):
    """(M, N, K) of the implicit GEMM of a stride-1 conv case in a direction"""
    n, h, w, c, k, ks, st, pad = case
    ho, wo = (T.conv_out_size(h, ks, st, pad)[0], T.conv_out_size(w, ks, st, pad)[0])
    if mode == 0:
        return n * ho * wo, k, ks * ks * c
    if mode == 1:
        return n * h * w, c, ks * ks * k
    return ks * ks * c, k, n * ho * wo


def clamped_split(K, bk, want):
    """the split-K factor a pinned `want` becomes: at most one k-tile per range, equal ranges, no empty range"""
    nk = max(1, -(-K // bk))
    want = max(1, min(want, nk))
    kps = -(-nk // want)
    return -(-nk // kps)


def streamk_grids(case, mode, cfg):
    """1, 3, 7 and one grid larger than tiles x k-tiles (or the 1024 the fix-up's contributor list holds)"""
    M, N, K = gemm_dims(case, mode)
    bm, bn = CFG_TILE[cfg]
    iters = -(-M // bm) * -(-N // bn) * -(-K // 32)
    return STREAMK_SMALL + (min(1024, iters + 3),)


def forced_f32_combos():
    """[(case, mode, cfg, 'splitk' | 'streamk', value)]: every configuration x direction x split of the float32 sweep.  The
    LDS-DMA staged forwards (9, 10) run whole K ranges or split-K slabs only: stream-K shares are their twins' (7, 8), swept
    under their own index."""
    out = []
    for case in FORCED_F32:
        for mode in MODES:
            for cfg in range(NUM_CFGS):
                out += [(case, mode, cfg, 'splitk', s) for s in SPLITS_F32]
                if not (mode == 0 and cfg in TWIN):
                    out += [(case, mode, cfg, 'streamk', g) for g in streamk_grids(case, mode, TWIN.get(cfg, cfg))]
    out += [(FORCED_STRIDED, mode, cfg, 'splitk', 1) for mode in MODES for cfg in range(NUM_CFGS)]
    return out


def forced_bf16_combos():
    """[(case, mode, 'bn' | 'ring', value, split)]"""
    out = [(case, mode, 'bn', bn, s) for case in FORCED_F32 for mode in MODES for bn in (64, 128) for s in SPLITS_BF16]
    for mode, (case, cfgs) in ((0, RING_FWD), (1, RING_BWD_D), (1, RING_BWD_D_96), (2, RING_BWD_F)):
        out += [(case, mode, 'ring', cfg, 0) for cfg in cfgs]
    return out


def forced_count():
    return len(forced_f32_combos()) + len(forced_bf16_combos())
