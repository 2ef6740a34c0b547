"""Shapes, templates and host-side conditions of tests/test_gpu_large_tensors.py (no GPU and no torch in here: tests/test_abi_large.py
builds every case on the CPU and asserts the conditions there too).

Template images.  Image i of every multi-GiB tensor is template i mod 7 of 7 small templates, so the float64 reference of 7 images
is the reference of the whole tensor, and the device compares EVERY image of an output with it.  A byte offset that wraps at 2^32,
or that is cut at 2^31, moves an access by 2^32 / image_bytes (2^31 / image_bytes) images: shift_condition() asserts that neither
is an integer multiple of 7, so the access lands on another template (or inside an image), never on a copy of the right one; the
templates of a tensor are asserted pairwise different.

Reductions over the batch (filter gradients) take dz = 0 except in chosen_images(): image 0, the images before / holding / after
byte 2^31 and byte 2^32 of the largest operand, and the last one.  A read that wraps, stops early or skips finds zeros or another
template and changes an integer result.

Operands are small integers as in tests/exact_ops.py and every sum of absolute products is asserted < 2^24 there
(E.require_headroom), so float32, bf16x3 and bf16 arithmetic are exact in any order and equality needs no tolerance."""
import functools

import numpy as np

import exact_ops as E
from oracle import tf13_ops as T

NT = 7                        # templates
LINE31, LINE32 = 1 << 31, 1 << 32
GUARD_BYTES = 1 << 16         # sentinel bytes in front of and behind every big output
MAX_ELEMS = (1 << 31) - 1     # check_desc: fewer than 2^31 - 1 elements per tensor


def shift_condition(what, image_bytes):
    """neither 2^31 / image_bytes nor 2^32 / image_bytes is an integer multiple of 7"""
    for line in (LINE31, LINE32):
        assert not (line % image_bytes == 0 and (line // image_bytes) % NT == 0), \
            f'{what}: an offset cut at {line} moves by {line // image_bytes} images of {image_bytes} bytes: a multiple of {NT}'


def distinct(what, templates):
    """the 7 templates of a tensor differ pairwise (a wrong image can only be right by being the right one)"""
    assert len(templates) == NT and len({np.ascontiguousarray(t).tobytes() for t in templates}) == NT, f'{what}: templates repeat'
    return templates


def chosen_images(n, image_bytes):
    """image 0, the images before / holding / after byte 2^31 and byte 2^32 of a tensor of n images, the last image"""
    out = {0, n - 1}
    for line in (LINE31, LINE32):
        hold = line // image_bytes
        out |= {i for i in (hold - 1, hold, hold + 1) if 0 <= i < n}
    return sorted(out)


def straddles(n, image_bytes, line):
    """does a tensor of n images end past byte `line`?"""
    return n * image_bytes > line


class ConvTemplates:
    """7 images of one conv layer, all three directions in float64.  y carries the bias; dz multiplies it."""

    def __init__(self, h, w, c, k, ks, st, pad, seed=0):
        self.geom = (h, w, c, k, ks, st, pad)
        self.what = f'conv templates {self.geom}'
        rng = np.random.default_rng(7100 + seed + h * w + c + k)
        self.x = E.ternary(rng, (NT, h, w, c))
        self.w = E.ternary(rng, (ks, ks, c, k))
        self.b = E.small_bias(rng, k)
        self.y = E.require_integers(self.what + ' y', T.conv2d_fwd(E.f64(self.x), E.f64(self.w), E.f64(self.b), st, pad))
        self.ho, self.wo = self.y.shape[1:3]
        self.dz = E.ternary(rng, self.y.shape)
        self.dx = E.require_integers(self.what + ' dx', T.conv2d_bwd_data(E.f64(self.dz), E.f64(self.w), self.x.shape, st, pad))
        E.require_headroom(self.what + ' forward', ks * ks * c, self.x, self.w, self.b)
        E.require_headroom(self.what + ' bwd-data', ks * ks * k, self.dz, self.w)
        self.relu_y = distinct(self.what + ' relu(y)', np.maximum(self.y, 0))
        self.masked_dx = distinct(self.what + ' dx (x > 0)', self.dx * (self.x > 0))
        distinct(self.what + ' x', self.x)
        distinct(self.what + ' dz', self.dz)
        self.rng = rng

    @functools.cached_property
    def pooled(self):
        """(pooled values, first-maximum bytes) of relu(y), per template"""
        pooled, arg = E.pool_reference(self.relu_y)
        distinct(self.what + ' pooled', pooled)
        distinct(self.what + ' argmax', arg)
        assert ((pooled == 0).mean() > 0.01), self.what + ': no ties at 0 in the pooled map'
        return pooled, arg

    def filter_grad(self, n, image_bytes):
        """-> (chosen images, their dz [len, ho, wo, k], dw, db): x is template-filled everywhere, dz zero outside the chosen"""
        h, w, c, k, ks, st, pad = self.geom
        imgs = chosen_images(n, image_bytes)
        rng = np.random.default_rng(7300 + n)
        dz = E.ternary(rng, (len(imgs), self.ho, self.wo, k))
        x = self.x[[i % NT for i in imgs]]
        dw, db = T.conv2d_bwd_filter(E.f64(x), E.f64(dz), (ks, ks, c, k), st, pad)
        E.require_headroom(self.what + ' bwd-filter', len(imgs) * self.ho * self.wo, x, dz)
        assert len(imgs) * self.ho * self.wo < E.F32_EXACT
        # every chosen image matters: without it some element of dw changes
        for j in range(len(imgs)):
            alone = T.conv2d_bwd_filter(E.f64(x[j:j + 1]), E.f64(dz[j:j + 1]), (ks, ks, c, k), st, pad)[0]
            assert alone.any(), f'{self.what}: chosen image {imgs[j]} adds nothing to dw'
        return imgs, dz, E.require_integers(self.what + ' dw', dw), E.require_integers(self.what + ' db', db)


@functools.lru_cache(maxsize=None)
def conv_templates(h, w, c, k, ks, st, pad, seed=0):
    return ConvTemplates(h, w, c, k, ks, st, pad, seed)


class PooledGradTemplates:
    """The pool-fused filter gradient (fewch.hip / fewch16.hip): x, the pooled activations and their argmax bytes are template-
    filled, the gradient of the pooled map is zero outside the chosen images."""

    def __init__(self, h, w, c, k, ks):
        self.geom = (h, w, c, k, ks)
        self.what = f'pooled filter-gradient templates {self.geom}'
        rng = np.random.default_rng(7500 + h * w + k)
        self.ho, self.wo = h - ks + 1, w - ks + 1
        self.ph, self.pw = self.ho // 2, self.wo // 2
        self.x = distinct(self.what + ' x', E.ternary(rng, (NT, h, w, c)))
        self.pooled = distinct(self.what + ' pooled', E.ternary(rng, (NT, self.ph, self.pw, k)))      # a third each: < 0, == 0, > 0
        self.arg = distinct(self.what + ' argmax', rng.integers(0, 4, (NT, self.ph, self.pw, k)).astype(np.uint8))

    def filter_grad(self, n, image_bytes):
        h, w, c, k, ks = self.geom
        imgs = chosen_images(n, image_bytes)
        rng = np.random.default_rng(7700 + n)
        dpool = E.ternary(rng, (len(imgs), self.ph, self.pw, k))
        t = [i % NT for i in imgs]
        dz = E.pool_grad_reference(self.arg[t], self.pooled[t], E.f64(dpool), (len(imgs), self.ho, self.wo, k), True)
        assert ((self.pooled[t] == 0) & (dpool != 0)).mean() > 0.1, 'ReluGrad edge not live'
        dw, db = T.conv2d_bwd_filter(E.f64(self.x[t]), dz, (ks, ks, c, k), 1, 'VALID')
        E.require_headroom(self.what, len(imgs) * self.ho * self.wo, self.x[t], dz)
        return imgs, dpool, E.require_integers(self.what + ' dw', dw), E.require_integers(self.what + ' db', db)


@functools.lru_cache(maxsize=None)
def pooled_grad_templates(h, w, c, k, ks):
    return PooledGradTemplates(h, w, c, k, ks)


class PoolTemplates:
    """The max pool family on post-ReLU integer activations (exact ties at 0 in most windows' neighbourhood) and, for the by-index
    gradients, recorded argmax bytes with pooled values of every sign."""

    def __init__(self, h, w, c):
        self.geom = (h, w, c)
        self.what = f'pool templates {self.geom}'
        rng = np.random.default_rng(7900 + h * w + c)
        self.x = distinct(self.what + ' x', np.maximum(E.integers(rng, (NT, h, w, c), 3), 0))
        self.y, self.first = E.pool_reference(E.f64(self.x))
        assert (self.y == 0).mean() > 0.01 and (self.first != 0).mean() > 0.3, self.what + ': ties at 0, maxima at every position'
        distinct(self.what + ' y', self.y)
        ph, pw = h // 2, w // 2
        self.dy = distinct(self.what + ' dy', E.ternary(rng, (NT, ph, pw, c)))
        self.dx = {relu: distinct(self.what + f' dx relu {relu}', E.pool_grad_reference(self.first, self.y, E.f64(self.dy), (NT, h, w, c), relu))
                   for relu in (True, False)}
        assert (self.dx[True] != self.dx[False]).any(), self.what + ': ReluGrad never bites'
        # by index: any bytes, pooled values of every sign
        self.arg = distinct(self.what + ' argmax', rng.integers(0, 4, (NT, ph, pw, c)).astype(np.uint8))
        self.pooled = distinct(self.what + ' pooled', E.ternary(rng, (NT, ph, pw, c)))
        self.dx_idx = {relu: distinct(self.what + f' dx by index relu {relu}',
                                      E.pool_grad_reference(self.arg, self.pooled, E.f64(self.dy), (NT, h, w, c), relu))
                       for relu in (True, False)}


@functools.lru_cache(maxsize=None)
def pool_templates(h, w, c):
    return PoolTemplates(h, w, c)


# ---- the shapes: the smallest that put an operand just past 2^32 bytes (bf16: 2^31) under 2^31 elements ----
GENERIC = dict(n=16500, h=64, w=64, c=16, k=16, ks=3, st=1, pad='SAME')           # x, y 4.33 GB float32, 2.16 GB bf16
GENERIC_LDY = 20                                                                  # the pitched forward: y 5.41 GB
RING_LDY = 24
# the LDS-DMA filter gradient addresses dz from the tensor's start: dz on both sides of 2^31 bytes, x (half as wide) under it
RING_BWD_F = dict(h=32, w=32, c=64, k=128, ks=3, st=1, pad='SAME')
RING_BWD_F_N = (8180, 8200)                                                       # dz 2 144 337 920 and 2 149 580 800 bytes
DCNF_FIRST = dict(h=100, w=100, c=3, k=64, ks=11, st=1, pad='VALID')
CONV3_N, CONV3_LDY = 2100, 72                                                     # y 4.35 GB (pitched 4.90)
# check_desc counts the UNPOOLED y of a pool-fused call too (n ho wo ldy < 2^31 - 1): 4142 images of this layer are the most it
# admits, their pooled map of 64 channels ends 270 848 bytes short of 2^31.  The pooled tensors pass 2^31 bytes by their pitch.
POOLED_N, POOLED_REFUSED_N = 4142, (4143, 8300)
CONV3_POOL_LD = 72                                                                # pooled map 2.42 GB, argmax bytes 0.54 GB
FEWCH_PLAIN_N = (1035, 1036)                                                      # dz 2 146 176 000 bytes, and past 2^31
FEWCH_POOLED_LD = {'f32': (64, 68), 'bf16': (128, 132)}                           # pooled gradient 2 147 212 800 / 2 281 413 600 (bf16: 2 214 313 200) bytes
STENCIL = dict(h=55, w=74, c=64)
STENCIL_N, STENCIL_MFMA_N, STENCIL_BOTH_N = 4200, (2061, 2062), (1030, 1031)     # x 4.37 GB; the MFMA form's 2 GiB, bwd_both's 1 GiB
POOL = dict(n=2100, h=90, w=90, c=64)                                             # 4.35 GB float32, 2.18 GB bf16
CAST_IMAGE = (4096, 64)                                                           # rows x row pitch of one template: 2^18 elements
CAST_N = 4100                                                                     # 1 074 790 400 elements: past 2^30
CHANNEL_PIXELS = 1 << 16                                                          # pixels per template of the channel copies


def image_bytes(pixels, ld, esz):
    return pixels * ld * esz


def fits(n, pixels, ld):
    return n * pixels * ld < MAX_ELEMS
