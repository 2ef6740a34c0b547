"""Exact-integer cases for every contraction route: inputs, float64 references, and the conditions that make element-by-
element equality with a float32 / bf16 kernel legitimate.  No GPU and no torch in here (test_exact_cpu.py builds every case
on the CPU; test_gpu_exact.py and exact_forced_worker.py run them).

Why equality needs no tolerance.  Operands are small integers (ternary {-1, 0, 1} unless a case says otherwise) and the
helper asserts, every time it builds a case,
  * every reference value is an integer,
  * K * max|a| * max|b| + max|bias| < 2^24 for the contraction length K of each direction (forward: r s c; bwd-data:
    r s k; bwd-filter: the pixel axis n ho wo) — or, where one operand is wide and that product form cannot hold, the
    actual maximum over the output elements of sum |a| |b| (the oracle contraction of the absolute values).  The bound is on
    the sum of ABSOLUTE products, so every partial sum of every k-tile, split-K slab, stream-K share and reduction order is
    an integer below 2^24 and therefore exact in float32,
  * an output a kernel stores as bf16 either has max|ref| <= 256 (bf16 holds every integer up to 256: nothing is rounded
    and a difference of 1 cannot hide), or is a rounded-store case: the reference is bf16_rne(exact integer), round to
    nearest with ties to even, bit for bit — at least a quarter of its elements are changed by the rounding and exact ties
    go up and down for both signs, so truncation, round-half-away and a double rounding all differ somewhere.
Operands are either integers <= 256 (exact as bf16: the hi plane of the bf16x3 split, whose lo plane is then zero), or WIDE:
integers up to 4000, which no bf16 holds in general.  A `bf16` kernel must then multiply bf16_rne(operand), and a `bf16x3`
kernel hi_a hi_b + hi_a lo_b + lo_a hi_b with hi = bf16_rne(a), lo = bf16_rne(a - hi) (12-bit integers: hi + lo = a
exactly), which the float64 oracle states as an integer again: with one operand wide and the other ternary it is the
unrounded contraction, with both wide it is the contraction minus that of the two lo planes.
These conditions are asserted on the CPU, every time a case is built, and no element is ever left out of a comparison.  One
thing is assumed of the hardware, and was checked on it: that the bf16 MFMA (v_mfma_f32_32x32x16_bf16) adds integer products exactly while every partial sum stays below 2^24, as the
float32 MFMA does.  The wide-operand cases, whose asserted bounds reach 1.39e7, are exact on the MI355X on every bf16 route
(bf16 and bf16x3, all three directions), so no magnitude had to be lowered."""
import copy
import functools

import numpy as np

from oracle import tf13_ops as T

F32_EXACT = 2 ** 24
BF16_EXACT = 256
X3_EXACT = 4095          # 12 bits: the hi (8 bits) and lo planes of the bf16x3 split hold such an integer exactly
WIDE_OPERAND = 4000      # a wide float32 operand: integers in [-4000, 4000]
ROUNDED_STORE_MAG = 8    # operands of the rounded-store cases (exact as bf16); their sums are far above 256
BOTH_WIDE = ('odd', 257, 511)      # odd integers of either sign in 257..511: bf16 ties, lo = +-1


def bf16_rne(a):
    """float32 -> the nearest bf16, ties to even, as float32: integer arithmetic on the bit pattern (NaN stays a quiet NaN)"""
    f = np.ascontiguousarray(a, dtype=np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    r = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    nan = (u & 0x7fffffff) > 0x7f800000
    r = np.where(nan, (u | 0x00400000) & 0xffff0000, r)
    return r.astype(np.uint32).view(np.float32).reshape(f.shape)


def bf16_split(a):
    """(hi, lo) of the bf16x3 split: hi = RNE(a), lo = RNE(a - hi) (the subtraction is exact in float32)"""
    f = np.ascontiguousarray(a, dtype=np.float32)
    hi = bf16_rne(f)
    return hi, bf16_rne(f - hi)


def rounding_census(exact):
    """of the integers a kernel stores as bf16 -> (rounded values, fraction the rounding changes, and the exact ties by
    (sign, direction): {('+', 'up'): count, ('+', 'down'): .., ('-', 'up'): .., ('-', 'down'): ..}; up = away from zero)"""
    e = f64(exact)
    r = f64(bf16_rne(e))
    ulp = np.ldexp(1.0, np.frexp(np.abs(e))[1] - 8)          # spacing of bf16 in the binade of |e|
    tie = (r != e) & (2 * np.abs(r - e) == ulp)
    up = np.abs(r) > np.abs(e)
    ties = {(sg, d): int((tie & (e > 0 if sg == '+' else e < 0) & (up if d == 'up' else ~up)).sum()) for sg in '+-' for d in ('up', 'down')}
    return r, float((r != e).mean()), ties


def require_rounding(what, exact, min_ties=10):
    """a rounded-store reference: -> bf16_rne(exact), having asserted that the rounding matters in it"""
    r, changed, ties = rounding_census(require_integers(what, f64(exact)))
    assert changed >= 0.25, f'{what}: the bf16 rounding changes only {changed:.1%} of the elements'
    assert min(ties.values()) >= min_ties, f'{what}: exact ties by sign and direction {ties}, fewer than {min_ties} of a kind'
    return r


def require_wide(what, a):
    """a wide operand: at least half of it is no bf16, with ties that go down (to an even neighbour below) and up"""
    r, changed, ties = rounding_census(a)
    assert amax(a) <= X3_EXACT, f'{what}: more than 12 bits, hi + lo of the bf16x3 split would not be exact'
    assert changed >= 0.5, f'{what}: {changed:.1%} of the operand is not representable in bf16, want half'
    assert ties['+', 'up'] + ties['-', 'up'] > 0 and ties['+', 'down'] + ties['-', 'down'] > 0, f'{what}: ties {ties}'


def ternary(rng, shape):
    return rng.integers(-1, 2, shape).astype(np.float32)


def integers(rng, shape, amax):
    """integers in [-amax, amax] (amax = 1: ternary)"""
    return rng.integers(-amax, amax + 1, shape).astype(np.float32)


def wide(rng, shape, amax):
    """integers in [-amax, amax] with, where there is room, the four ties 257 / 259 (down / up to even) of both signs planted"""
    a = rng.integers(-amax, amax + 1, shape).astype(np.float32)
    if a.size >= 8:
        a.reshape(-1)[rng.choice(a.size, 4, replace=False)] = (257, 259, -257, -259)
    return a


def operand(rng, shape, mag):
    """mag: an integer bound (above 256: a wide operand), or ('odd', lo, hi): odd integers of either sign in lo..hi"""
    if isinstance(mag, tuple):
        kind, lo, hi = mag
        assert kind == 'odd' and lo % 2 == 1 and hi % 2 == 1
        return ((2 * rng.integers(lo // 2, hi // 2 + 1, shape) + 1) * rng.choice((-1, 1), shape)).astype(np.float32)
    return integers(rng, shape, mag) if mag <= BF16_EXACT else wide(rng, shape, mag)


def small_bias(rng, k):
    return rng.integers(-3, 4, k).astype(np.float32)


def amax(a):
    return float(np.abs(a).max()) if a.size else 0.0


def require_integers(what, a):
    assert np.array_equal(a, np.rint(a)), f'{what}: the reference is not integer-valued'
    return a


def require_headroom(what, K, a, b, bias=None, contract=None, factor=1.0, limit=BF16_EXACT):
    """-> the bound on the sum of absolute products (+ bias), times `factor` (a scale the epilogue multiplies by), asserted
    < 2^24: K max|a| max|b| where that holds, else — given contract(a, b), the oracle contraction of the direction — the
    actual maximum over the output elements of sum |a| |b|.  Either covers every partial sum in every order.  limit: 256
    (operands exact in bf16) or 4095 (wide operands: the bound is then taken on |hi| + |lo| of the bf16x3 split, which
    covers RNE(a) = hi for a `bf16` kernel and the three hi / lo products of a `bf16x3` kernel)."""
    extra = amax(bias) if bias is not None else 0.0
    assert amax(a) <= limit and amax(b) <= limit, f'{what}: operands are not exact in bf16' if limit == BF16_EXACT else f'{what}: operands above {limit}'
    if limit > BF16_EXACT:      # |hi| + |lo| >= |RNE(a)|: what a kernel that rounds or splits the operand multiplies
        a, b = (sum(np.abs(f64(p)) for p in bf16_split(v)) for v in (a, b))
    bound = factor * K * amax(a) * amax(b) + extra
    if bound >= F32_EXACT and contract is not None:
        bound = factor * amax(contract(np.abs(f64(a)), np.abs(f64(b)))) + extra
    assert bound < F32_EXACT, f'{what}: sum of absolute products may reach {bound} >= 2^24'
    return bound


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
    """One convolution, all three directions.  y is the pre-activation output WITH the bias; dz multiplies it.
    mags = (x, w, dz): a magnitude per operand (operand()), where one of them is wide; mag: the same for all three."""
    rounds = False       # True in a rounded-store view: a bf16 tensor holds bf16_rne(reference)

    def __init__(self, n, h, w, c, k, ks, st, pad, mag=1, mags=None):
        self.shape = (n, h, w, c, k, ks, st, pad)
        self.what = f'conv {self.shape} |operands| <= {mag}' if mags is None else f'conv {self.shape} x, w, dz of magnitude {mags}'
        self.mags = xm, wm, dm = mags or (mag, mag, mag)
        limit = BF16_EXACT if mags is None else X3_EXACT
        rng = np.random.default_rng(5000 + h * w + c + k)
        self.x = operand(rng, (n, h, w, c), xm)
        self.w = operand(rng, (ks, ks, c, k), wm)
        self.b = small_bias(rng, k)
        self.y = require_integers(self.what + ' y', self.fwd(self.x, self.w, self.b))
        self.ho, self.wo = self.y.shape[1:3]
        self.dz = operand(rng, self.y.shape, dm)
        dw, db = self.bwd_filter(self.x, self.dz)
        self.dw, self.db = require_integers(self.what + ' dw', dw), require_integers(self.what + ' db', db)
        self.dx = require_integers(self.what + ' dx', self.bwd_data(self.dz, self.w))
        self.headroom = (require_headroom(self.what + ' forward', ks * ks * c, self.x, self.w, self.b, self.fwd, limit=limit),
                         require_headroom(self.what + ' bwd-data', ks * ks * k, self.dz, self.w, None, self.bwd_data, limit=limit),
                         require_headroom(self.what + ' bwd-filter', n * self.ho * self.wo, self.x, self.dz, None,
                                          lambda x, dz: self.bwd_filter(x, dz)[0], limit=limit))
        assert amax(self.db) < F32_EXACT and n * self.ho * self.wo * amax(self.dz) < F32_EXACT, self.what + ' db'

    # the oracle's contractions of this geometry, in float64
    def fwd(self, x, w, b=None):
        return T.conv2d_fwd(f64(x), f64(w), None if b is None else f64(b), self.shape[6], self.shape[7])

    def bwd_filter(self, x, dz):
        n, h, w, c, k, ks, st, pad = self.shape
        return T.conv2d_bwd_filter(f64(x), f64(dz), (ks, ks, c, k), st, pad)

    def bwd_data(self, dz, w):
        n, h, ww, c, k, ks, st, pad = self.shape
        return T.conv2d_bwd_data(f64(dz), f64(w), (n, h, ww, c), st, pad)

    def view(self, what, **refs):
        """this case with other references (same operands)"""
        v = copy.copy(self)
        v.__dict__.pop('pooled', None)
        v.__dict__.update(refs, what=f'{self.what}, {what}')
        return v

    def bf16(self, *names):
        """the named outputs are stored as bf16 somewhere: hold them to 256 (not for a rounded-store view, whose callers ask
        `rounds` first)"""
        for name in names:
            require_bf16(f'{self.what} {name}', getattr(self, name))
        return self

    def stored(self, name, ref):
        """what a bf16 tensor holds of the reference `ref`: itself, asserted <= 256 — or, in a rounded-store view, its RNE"""
        return f64(bf16_rne(ref)) if self.rounds else require_bf16(f'{self.what} {name}', ref)

    @functools.cached_property
    def pooled(self):
        """(pooled, argmax) of relu(y)"""
        return pool_reference(np.maximum(self.y, 0))

    def rounded_store(self, *names):
        """The view in which bf16 tensors hold bf16_rne(reference): the named references (those the test stores as bf16) are
        asserted to be changed by the rounding in a quarter of their elements, with >= 10 exact ties up and down for each sign.
        Of a strided dx the quarter is taken over the pixels that receive a tap at all: the others are exact zeros by the
        geometry (three quarters of the 1 x 1 stride-2 case), which no rounding could change."""
        assert max(self.mags) <= BF16_EXACT, 'rounded-store cases have operands that are exact in bf16'
        for name in names:
            ref = getattr(self, name)
            if name == 'dx' and self.shape[6] > 1:
                tapped = self.bwd_data(np.ones_like(self.dz), np.ones_like(self.w)) != 0
                assert not ref[~tapped].any()
                ref = ref[tapped]
            require_rounding(f'{self.what} {name}', ref)
        return self.view('bf16 tensors hold RNE(reference)', rounds=True)

    @functools.cached_property
    def arith_bf16(self):
        """The view a `bf16` kernel on float32 tensors must produce: the oracle on bf16_rne(operand).  db is the sum of the
        UNROUNDED dz: the kernel adds its float32 registers before they are converted (igemm_bf16.h, `bsum[e] += rb[j][e]`)."""
        for name, m in zip(('x', 'w', 'dz'), self.mags):
            if not isinstance(m, tuple) and m > BF16_EXACT:
                require_wide(f'{self.what} {name}', getattr(self, name))
        x, w, dz = (bf16_rne(v) for v in (self.x, self.w, self.dz))
        return self.view('operands rounded to bf16', y=self.fwd(x, w, self.b), dw=self.bwd_filter(x, dz)[0], dx=self.bwd_data(dz, w))

    @functools.cached_property
    def arith_bf16x3(self):
        """The view a `bf16x3` kernel must produce: hi_a hi_b + hi_a lo_b + lo_a hi_b = a b - lo_a lo_b (a = hi + lo exactly).
        One operand wide, the other ternary (lo = 0): the unrounded oracle.  Both wide: the omitted term is asserted non-zero
        in at least half of the output elements, so a kernel that keeps it, or that splits by truncation, differs."""
        (_, lx), (_, lw), (_, ldz) = (bf16_split(v) for v in (self.x, self.w, self.dz))
        for v in (self.x, self.w, self.dz):
            hi, lo = bf16_split(v)
            assert np.array_equal(f64(hi) + f64(lo), f64(v)), self.what + ': hi + lo is not the operand'
        omitted = self.fwd(lx, lw), self.bwd_filter(lx, ldz)[0], self.bwd_data(ldz, lw)
        if sum(isinstance(m, tuple) for m in self.mags) == 3:
            assert all((np.abs(lo) == 1).all() for lo in (lx, lw, ldz)), self.what + ': lo planes'
            for name, o in zip(('y', 'dw', 'dx'), omitted):
                assert (o != 0).mean() >= 0.5, f'{self.what} {name}: the lo lo term is zero in {1 - (o != 0).mean():.1%} of the elements'
        else:
            assert not any(o.any() for o in omitted), self.what + ': one operand wide, lo lo must vanish'
        return self.view('bf16x3 split', y=self.y - omitted[0], dw=self.dw - omitted[1], dx=self.dx - omitted[2])


@functools.lru_cache(maxsize=None)
def conv_case(n, h, w, c, k, ks, st, pad, mag=1, mags=None):
    return ConvCase(n, h, w, c, k, ks, st, pad, mag, mags)


def wide_variants(case):
    """[(name, ConvCase)]: x wide and the rest ternary, w wide, dz wide — each operand's conversion isolated in each direction"""
    return [(name, conv_case(*case, mags=tuple(WIDE_OPERAND if o == name else 1 for o in ('x', 'w', 'dz')))) for name in ('x', 'w', 'dz')]


def rounded_pool(cs, y, floor=10):
    """(pooled, argmax) over the bf16-rounded activations `y`: the first maximum of the ROUNDED window.  Asserts that in at
    least 10 windows that is another position than the first maximum of the unrounded window (the rounding created a tie).
    floor = 0 only for the two cases of POOL_NO_TIES below."""
    pooled, arg = pool_reference(f64(bf16_rne(y)))
    moved = int((arg != pool_reference(y)[1]).sum())
    assert moved >= floor, f'{cs.what}: rounding moves the first maximum in only {moved} windows'
    return pooled, arg


class BothCase:
    """A one-filter 5x5 stride-1 conv on a buffer of pixel stride ldx >= c (stencil1.hip)"""

    def __init__(self, n, h, w, c, pad, ldx, lddx, mag=1):
        self.shape = (n, h, w, c, pad, ldx, lddx)
        self.what = f'one-filter conv {self.shape}' + (f' |operands| <= {mag}' if mag != 1 else '')
        rng = np.random.default_rng(5700 + n * h * w + c)
        self.xbuf = integers(rng, (n, h, w, ldx), mag)
        self.x = self.xbuf[..., :c]
        self.w = integers(rng, (5, 5, c, 1), mag)
        self.b = small_bias(rng, 1)
        self.y = require_integers(self.what + ' y', T.conv2d_fwd(f64(self.x), f64(self.w), f64(self.b), 1, pad))
        self.dz = integers(rng, self.y.shape, mag)
        dw, db = T.conv2d_bwd_filter(f64(self.x), f64(self.dz), self.w.shape, 1, pad)
        self.dw, self.db = require_integers(self.what + ' dw', dw), require_integers(self.what + ' db', db)
        self.dx = require_integers(self.what + ' dx', T.conv2d_bwd_data(f64(self.dz), f64(self.w), self.x.shape, 1, pad))
        require_headroom(self.what + ' forward', 25 * c, self.x, self.w, self.b)
        require_headroom(self.what + ' bwd-data', 25, self.dz, self.w)
        require_headroom(self.what + ' bwd-filter', n * self.y.shape[1] * self.y.shape[2], self.x, self.dz)
        # what a bf16 dx holds: dx itself (ternary operands: <= 256), or its RNE where the 25-tap sums are far above 256
        self.dx16 = require_bf16(self.what + ' dx', self.dx) if mag == 1 else require_rounding(self.what + ' dx', self.dx)


@functools.lru_cache(maxsize=None)
def both_case(*shape, mag=1):
    return BothCase(*shape, mag=mag)


class PooledBwdfCase:
    """Filter gradient of conv -> ReLU -> 2x2 max pool from the gradient of the POOLED map (fewch.hip / fewch16.hip): ternary
    `pooled` makes a third of the maxima exactly 0 and a third negative, so ReluGrad's edge `> 0` is held exactly"""

    def __init__(self, n, h, w, c, k, ks, st, ld, lda, xmag=1):
        self.shape = (n, h, w, c, k, ks, st, ld, lda)
        self.what = f'pool-fused filter gradient {self.shape}' + (f' |x| <= {xmag}' if xmag != 1 else '')
        rng = np.random.default_rng(5900 + h * w + k)
        self.x = operand(rng, (n, h, w, c), xmag)
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
        require_headroom(self.what, n * self.ho * self.wo, self.x, self.dz, limit=BF16_EXACT if xmag == 1 else X3_EXACT)
        if xmag > BF16_EXACT:      # what a `bf16` kernel that converts the float32 image itself must produce (fewch16.hip)
            require_wide(self.what + ' x', self.x)
            self.dw16 = require_integers(self.what + ' dw', T.conv2d_bwd_filter(f64(bf16_rne(self.x)), self.dz, (ks, ks, c, k), st, 'VALID')[0])
            assert (self.dw16 != self.dw).mean() > 0.5


@functools.lru_cache(maxsize=None)
def pooled_bwdf_case(*shape, xmag=1):
    return PooledBwdfCase(*shape, xmag=xmag)


class DenseCase:
    """mags = (x, w, dz) as in ConvCase; scales: the factors dense_bwd_data multiplies dx by, held in the headroom"""

    def __init__(self, m, k, n, mags=None, scales=(2.0,)):
        self.shape = (m, k, n)
        self.what = f'dense {self.shape}' + (f' x, w, dz of magnitude {mags}' if mags else '')
        self.mags = xm, wm, dm = mags or (1, 1, 1)
        limit = BF16_EXACT if mags is None else X3_EXACT
        rng = np.random.default_rng(5300 + m + k + n)
        self.x = operand(rng, (m, k), xm)
        self.w = operand(rng, (k, n), wm)
        self.b = small_bias(rng, n)
        self.keep = rng.random((m, n)) >= 0.5
        self.dz = operand(rng, (m, n), dm)
        self.y = require_integers(self.what + ' y', f64(self.x) @ f64(self.w) + f64(self.b))
        self.dx = require_integers(self.what + ' dx', f64(self.dz) @ f64(self.w).T)
        self.dw = require_integers(self.what + ' dw', f64(self.x).T @ f64(self.dz))
        self.db = require_integers(self.what + ' db', f64(self.dz).sum(0))
        require_headroom(self.what + ' forward', k, self.x, self.w, 2 * self.b, lambda a, b: a @ b, limit=limit)      # (dropout doubles: still exact)
        require_headroom(self.what + ' bwd-data', n, self.dz, self.w, None, lambda a, b: a @ b.T, factor=max(scales), limit=limit)
        require_headroom(self.what + ' bwd-filter', m, self.x, self.dz, None, lambda a, b: a.T @ b, limit=limit)
        assert m * amax(self.dz) < F32_EXACT

    def bf16(self):
        """dense_fwd_ex's bf16 second output (relu, dropout x 2) and dense_bwd_data_ex's bf16 dx (scale 2)"""
        require_bf16(self.what + ' 2 y', 2 * self.y)
        require_bf16(self.what + ' 2 dx', 2 * self.dx)
        return self

    def rounded_store(self):
        """bf16 tensors hold RNE(reference): asserted to matter in y and dx (and so in 2 y and 3 dx: test_exact_cpu.py)"""
        require_rounding(self.what + ' y', self.y)
        require_rounding(self.what + ' dx', self.dx)
        return self


@functools.lru_cache(maxsize=None)
def dense_case(m, k, n, mags=None, scales=(2.0,)):
    return DenseCase(m, k, n, mags, scales)


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


# ---- rounded stores: operands up to 8 (exact as bf16), bf16 tensors hold RNE(reference) ----
# The GENERIC cases whose tensors can be bf16, but for (1, 1, 1, 16, 8, 1, 1): its 8 outputs cannot hold 10 ties of each kind.
ROUNDED_GENERIC = [c for c in GENERIC if stores_bf16(c) and c[:3] != (1, 1, 1)]
# ... and every GUARD case, on float32 inputs with a bf16 output (STORE_Y alone).  The last one, k = 4 at a pitch of 12 bf16 (24
# bytes: rows that are no whole 16-byte pieces, an N tail of 4 columns in a 32-wide tile), needs operands up to 16 (ROUNDED_MAG)
ROUNDED_GUARD = list(GUARD)
ROUNDED_BOTH = (BOTH[0], 64)          # one-filter stencil: 25-tap sums need operands up to 64 to lie far above 256
# bf16 arithmetic on float32 tensors, both operands wide (odd integers in 257..511): a K that keeps 2^24
BOTH_WIDE_CASES = [(1, 10, 11, 4, 12, 3, 2, 'SAME'), (1, 1, 1, 16, 8, 1, 1, 'VALID')]
# dense.hip's bf16 streaming form (the fused filter gradient + Adam): 32 < m <= 64, rows of x in 16-byte pieces, columns in 8- and
# 16-byte pieces; 45 rows: the last 16-row step of the batch axis is partial
DENSE_STREAM_BF16 = [(45, 1028, 1030), (64, 516, 1032)]


# cases whose sums at magnitude 8 stay too close to 256 for a quarter of them to be rounded (short K: operands up to 32), or
# for the rounding to move the first maximum of 10 pool windows (the third: 6 windows at magnitude 8, 13 at 16)
ROUNDED_MAG = {(20, 31, 33, 64, 48, 3, 2, 'SAME'): 32, (2, 17, 20, 3, 16, 5, 2, 'VALID'): 32, (2, 21, 30, 32, 64, 3, 1, 'VALID'): 16,
               (1, 9, 11, 16, 4, 3, 1, 'SAME'): 16, (3, 9, 10, 8, 8, 1, 2, 'VALID'): 32}
# strided bwd-data as one launch: of the 1 x 1 case a quarter of the pixels receive a tap (rounded_store takes the condition over
# them: 55 % rounded at magnitude 32); the rounded stores then lie next to the exact zeros of the other classes
ROUNDED_STRIDED = list(STRIDED_ONE_LAUNCH_BF16)


# The one image case below 33 filters (the bf16 implicit GEMM's pooling epilogue): its 384 windows of stride-2 outputs share few
# taps, rounding moves no first maximum in them (nor in 4 x 33 x 40 x 32 filters at magnitudes 8 .. 32: 4 at most).  Its
# pooled map and bytes are still held bit for bit; the tie condition is asserted on every other pool case.
POOL_SMALL_IMAGE = (2, 17, 20, 3, 16, 5, 2, 'VALID')
# ... and the smallest GUARD case: 80 windows, none moved at magnitude 16 or 32
POOL_SMALL_GUARD = (1, 9, 11, 16, 4, 3, 1, 'SAME')
POOL_NO_TIES = (POOL_SMALL_IMAGE, POOL_SMALL_GUARD)


def rounded_case(case, *names):
    """names: the references the test stores as bf16 ('y', 'dx')"""
    return conv_case(*case[:8], ROUNDED_MAG.get(tuple(case[:8]), ROUNDED_STORE_MAG)).rounded_store(*names)


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


def forced_bf16_rounded_combos():
    """the pinned bf16 launches that store a bf16 result (forward and bwd-data; the filter gradient stays float32), again on the
    rounded-store form of their case: a split-K launch must round ONCE, after the slabs are added"""
    return [combo for combo in forced_bf16_combos() if combo[1] != 2]


def forced_count():
    return len(forced_f32_combos()) + len(forced_bf16_combos()) + len(forced_bf16_rounded_combos())


# ---- operands off the 16-byte grid (test_gpu_exact_offgrid.py) ----
# include/a3d.h lets a float32 tensor, a bias or an argmax row start at any multiple of its element size; the front end routes by
# address & 15 of every operand.  Byte offsets past a 256-byte boundary, by element type:
OFFGRID_BYTES = {'f32': (4, 8, 12), 'bf16': (2, 4, 8), 'u8': (1, 4, 8)}
OFFGRID_ALONE = 4                                       # sweep 1: each pointer operand alone (every type has this offset)
OFFGRID_IMAGE = 8                                       # sweep 2: the image-side operand alone: 8-byte runs, b64 staging
OFFGRID_TOGETHER = {'f32': 12, 'bf16': 2, 'u8': 1}      # sweep 3: all operands at once, each at the offset of its type not used above
OFFGRID_WS = (16, 4)                                    # sweep 4: the workspace off the 256-byte grid, and off the 16-byte one
ELEMENT_BYTES = {'f32': 4, 'bf16': 2, 'u8': 1}

# entry (a key of the test's launchers) -> (the C entry point, its pointer operands in argument order, the image-side operand).
# An operand's element type is 'f32' unless the launch's `types` names another.
OFFGRID_ENTRIES = {
    'conv2d_fwd': ('a3d_conv2d_fwd', ('x', 'w', 'bias', 'y'), 'x'),                       # bias + ReLU
    'conv2d_pool_fwd': ('a3d_conv2d_pool_fwd', ('x', 'w', 'bias', 'y', 'argmax'), 'x'),
    'conv2d_bwd_data': ('a3d_conv2d_bwd_data', ('dz', 'w', 'dx'), 'dx'),
    'conv2d_bwd_data_mask': ('a3d_conv2d_bwd_data', ('dz', 'w', 'dx', 'mask'), 'dx'),
    'conv2d_bwd_filter': ('a3d_conv2d_bwd_filter', ('x', 'dz', 'dw'), 'x'),
    'conv2d_bwd_filter_db': ('a3d_conv2d_bwd_filter', ('x', 'dz', 'dw', 'db'), 'x'),
    'conv2d_bwd_filter_pooled': ('a3d_conv2d_bwd_filter_pooled', ('x', 'dpool', 'pooled', 'argmax', 'dw', 'db'), 'x'),
    'conv2d_bwd_both': ('a3d_conv2d_bwd_both', ('x', 'dz', 'w', 'dw', 'db', 'dx'), 'x'),
    'dense_fwd': ('a3d_dense_fwd', ('x', 'w', 'bias', 'y', 'drop_keep'), 'x'),
    'dense_bwd_data': ('a3d_dense_bwd_data', ('dz', 'w', 'dx', 'mask'), 'dx'),
    'dense_bwd_filter': ('a3d_dense_bwd_filter', ('x', 'dz', 'dw', 'db'), 'x'),
    'dense_bwd_filter_adam_tf1': ('a3d_dense_bwd_filter_adam_tf1', ('var_w', 'm_w', 'v_w', 'dz', 'x'), None),
    'dense_fwd_ex': ('a3d_dense_fwd_ex', ('x', 'w', 'bias', 'y', 'drop_keep'), 'x'),
    'dense_bwd_data_ex': ('a3d_dense_bwd_data_ex', ('dz', 'w', 'dx', 'mask'), 'dx'),
}
U8_OPERANDS = ('argmax', 'drop_keep')

# the smallest shapes that still reach each route, all from the tables above
OFFGRID_GENERIC = [(1, 9, 11, 16, 4, 3, 1, 'SAME'), (3, 13, 18, 32, 200, 3, 1, 'SAME')]      # generic fp32 GEMM, vec4-capable
OFFGRID_GLDS_FROM = GENERIC                    # ... and the smallest of these whose on-grid forward is LDS-DMA staged (found on the GPU)
OFFGRID_STRIDED = [STRIDED_ONE_LAUNCH[0]]
OFFGRID_FEW_CHANNEL = [FEW_CHANNEL[1], FEW_CHANNEL[3], FEW_CHANNEL[2], FEW_CHANNEL[4]]      # conv3, window runs, fewch
OFFGRID_POOL = [(2, 40, 52, 3, 63, 9, 2, 'VALID')] + [g[:6] + (1, 'SAME') for g in (GUARD[3], GUARD[2])]
OFFGRID_POOLED_BWDF = [POOLED_BWDF[1]]
OFFGRID_BOTH = [BOTH[0], BOTH[5], BOTH[2]]     # 64 channels SAME, 64 channels VALID, the 40-channel VALID case
OFFGRID_BOTH_FWD = [BOTH[0], BOTH[5]]
OFFGRID_BOTH_BWD_F = [BOTH[0]]
OFFGRID_BF16_STORED = [RING_FWD[0]]            # (2, 13, 18, 64, 200, 3, 1, 'SAME')
OFFGRID_BF16_ARITH = [OFFGRID_GENERIC[1]]      # bf16 / bf16x3 arithmetic on float32 tensors, E.wide_variants operands
OFFGRID_DENSE = [DENSE[0], DENSE[1], DENSE[6]]
OFFGRID_DENSE_ADAM = [(32, 384, 520), DENSE_STREAM_BF16[0]]
OFFGRID_DENSE_BF16 = [DENSE_BF16[0]]
assert OFFGRID_POOL[0][:7] == POOLED_BWDF[1][:7] and OFFGRID_BF16_STORED[0] == (2, 13, 18, 64, 200, 3, 1, 'SAME')
assert all(c in GENERIC + [g[:6] + (1, 'SAME') for g in GUARD] for c in OFFGRID_GENERIC) and OFFGRID_STRIDED[0][6] == 2


def operand_type(name, types=None):
    return (types or {}).get(name, 'u8' if name in U8_OPERANDS else 'f32')


def offgrid_sweep(entry, types=None, ws=True):
    """[(label, {operand: byte offset}, workspace byte offset)] of one entry point: each operand alone at +4 bytes, the image-side
    operand alone at +8, all operands together (float32 +12, bf16 +2, uint8 +1), then the workspace at +16 and +4 under on-grid
    operands.  The first element is the on-grid launch the others are compared with."""
    _, operands, image = OFFGRID_ENTRIES[entry]
    for o in operands:
        assert OFFGRID_ALONE in OFFGRID_BYTES[operand_type(o, types)] and OFFGRID_IMAGE in OFFGRID_BYTES[operand_type(o, types)]
    out = [('on-grid', {}, 0)]
    out += [(f'{o}+{OFFGRID_ALONE}', {o: OFFGRID_ALONE}, 0) for o in operands]
    if image is not None:
        out.append((f'{image}+{OFFGRID_IMAGE}', {image: OFFGRID_IMAGE}, 0))
        out.append(('all', {o: OFFGRID_TOGETHER[operand_type(o, types)] for o in operands}, 0))
    if ws:
        out += [(f'ws+{b}', {}, b) for b in OFFGRID_WS]
    for _, offs, _ in out:
        for o, b in offs.items():
            t = operand_type(o, types)
            assert b in OFFGRID_BYTES[t] and b % ELEMENT_BYTES[t] == 0 and b % 16 != 0
    return out


def offgrid_offsets_used():
    """every byte offset of OFFGRID_BYTES is used by some sweep"""
    used = {t: {OFFGRID_ALONE, OFFGRID_IMAGE, OFFGRID_TOGETHER[t]} for t in OFFGRID_BYTES}
    return all(used[t] == set(OFFGRID_BYTES[t]) for t in OFFGRID_BYTES)


# What include/a3d.h says an entry point refuses: (C entry point, operand) -> the alignment in bytes its text asks of that operand
# (float32 unless the key names the bf16 form).  Written from the header's alignment paragraph, not from the code: a launch whose
# operand breaks one of these must return A3D_EINVAL before anything is enqueued, every other placement must be accepted.
REFUSED = {
    # "`ws` ... 16-byte aligned", every entry point with a workspace argument but the one below
    **{(e, 'ws'): 16 for e in ('a3d_conv2d_fwd', 'a3d_conv2d_pool_fwd', 'a3d_conv2d_bwd_data', 'a3d_conv2d_bwd_filter',
                               'a3d_conv2d_bwd_filter_pooled', 'a3d_dense_fwd', 'a3d_dense_bwd_data', 'a3d_dense_bwd_filter',
                               'a3d_dense_fwd_ex', 'a3d_dense_bwd_data_ex')},
    # a3d_conv2d_bwd_both: x, w and a float32 dx on a channel pair (8 bytes), a bf16 dx on a pair of its own (4), ws on 4
    ('a3d_conv2d_bwd_both', 'x'): 8, ('a3d_conv2d_bwd_both', 'w'): 8, ('a3d_conv2d_bwd_both', 'dx'): 8,
    ('a3d_conv2d_bwd_both', 'dx:bf16'): 4, ('a3d_conv2d_bwd_both', 'ws'): 4,
    # a3d_conv2d_bwd_filter_pooled: x in 16-byte pieces; dpool / pooled in whole 4-channel groups: 16 bytes float32, 8 bytes bf16
    ('a3d_conv2d_bwd_filter_pooled', 'x'): 16, ('a3d_conv2d_bwd_filter_pooled', 'dpool'): 16,
    ('a3d_conv2d_bwd_filter_pooled', 'pooled'): 16, ('a3d_conv2d_bwd_filter_pooled', 'dpool:bf16'): 8,
    ('a3d_conv2d_bwd_filter_pooled', 'pooled:bf16'): 8,
    # bf16 tensors (A3D_STORE_*): base 16-byte aligned, whichever entry point reads or writes them
    **{(e, o + ':bf16'): 16 for e, ops in (('a3d_conv2d_fwd', ('x', 'w', 'y')), ('a3d_conv2d_bwd_data', ('dz', 'w', 'dx', 'mask')),
                                            ('a3d_conv2d_bwd_filter', ('x', 'dz')), ('a3d_dense_fwd_ex', ('x', 'w')),
                                            ('a3d_dense_bwd_data_ex', ('dz', 'w', 'dx', 'mask'))) for o in ops},
    # a3d_dense_fwd_ex on a bf16 x: the float32 y is written in 16-byte pieces by the LDS-DMA kernel, the only one that reads a bf16 x
    ('a3d_dense_fwd_ex', 'y'): 16,
}


def refused_operands(entry, offsets, ws_off, types=None):
    """the operands of this placement that include/a3d.h lets the entry point refuse (REFUSED), in argument order"""
    cname, operands, _ = OFFGRID_ENTRIES[entry]
    bad = []
    for o in operands:
        t = operand_type(o, types)
        need = REFUSED.get((cname, o if t in ('f32', 'u8') else f'{o}:{t}'))
        if need and offsets.get(o, 0) % need:
            bad.append(o)
    need = REFUSED.get((cname, 'ws'))
    if need and ws_off % need:
        bad.append('ws')
    return bad
