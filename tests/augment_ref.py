"""Host reference (numpy only) of a3d_warp_bilinear_pair: the per-element contract of include/a3d.h restated float32
operation by operation.  numpy rounds every float32 operation once and never contracts a multiply and an add, which is
what the contract asks of the kernel.  tests/test_augment_cpu.py pins it to the oracle's resize, to flips and slices;
tests/test_gpu_augment.py holds the kernel to it bit for bit."""
import numpy as np

STRIDE = 12
F = np.float32


def u8_lut():
    """Pixel value k -> fl(fl(fl(k / 255) - 0.5) + 0.5): the float the converter and the loader's `+ 0.5` produce."""
    k = np.arange(256, dtype=np.float32)
    return ((k / F(255)) - F(0.5)) + F(0.5)


def as_float(x):
    return u8_lut()[x] if x.dtype == np.uint8 else x


def coords(table, h, w, oh, ow):
    """Clamped float32 source coordinates (u', v'), each [n, oh, ow], of every output pixel."""
    t = np.asarray(table, np.float32)
    sx, sy = F(w) / F(ow), F(h) / F(oh)
    u = (np.arange(ow, dtype=np.float32) * sx)[None, None, :]
    v = (np.arange(oh, dtype=np.float32) * sy)[None, :, None]
    m = [t[:, j][:, None, None] for j in range(6)]
    with np.errstate(invalid='ignore', over='ignore'):
        fx = ((m[0] * u) + (m[1] * v)) + m[2]
        fy = ((m[3] * u) + (m[4] * v)) + m[5]
    assert fx.dtype == np.float32 and fy.dtype == np.float32
    # fmaxf / fminf return the operand that is a number: a NaN coordinate lands on 0
    fx = np.fmin(np.fmax(fx, F(0)), F(w - 1))
    fy = np.fmin(np.fmax(fy, F(0)), F(h - 1))
    return fx, fy


def warp(x, table, oh, ow, second=False):
    """x [n, h, w, c] float32 or uint8 -> [n, oh, ow, c] float32.  second: the tensor takes the depth gain (column 10) on
    every channel instead of the per-channel gains (columns 6..9)."""
    n, h, w, c = x.shape
    t = np.asarray(table, np.float32)
    assert t.shape == (n, STRIDE) and (second or c <= 4)
    xf = as_float(x)
    fx, fy = coords(t, h, w, oh, ow)
    x0 = fx.astype(np.int64)
    y0 = fy.astype(np.int64)
    x1 = np.minimum(x0 + 1, w - 1)
    y1 = np.minimum(y0 + 1, h - 1)
    lx = (fx - x0.astype(np.float32))[..., None]
    ly = (fy - y0.astype(np.float32))[..., None]
    b = np.arange(n)[:, None, None]
    with np.errstate(invalid='ignore', over='ignore'):
        tl, tr = xf[b, y0, x0], xf[b, y0, x1]
        bl, br = xf[b, y1, x0], xf[b, y1, x1]
        top = tl + (tr - tl) * lx
        bot = bl + (br - bl) * lx
        out = top + (bot - top) * ly
        gain = np.broadcast_to(t[:, 10:11], (n, c)) if second else t[:, 6:6 + c]
        y = out * gain[:, None, None, :]
    assert y.dtype == np.float32
    return y


def identity(n):
    t = np.zeros((n, STRIDE), np.float32)
    t[:, [0, 4, 6, 7, 8, 9, 10]] = 1
    return t


def window_corners(p, h, w):
    """The four corners of the sampled window of each image, float64 [n, 4, 2] (x, y), recomputed from draw()'s (r, s, t):
    the images of the corners of [0, w-1] x [0, h-1] under p' = c + t + R(r) diag(flip, 1) (p - c) / s."""
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float64) - [cx, cy]
    c_, s_ = np.cos(p['r'])[:, None], np.sin(p['r'])[:, None]
    dx = corners[None, :, 0] * p['flip'][:, None] / p['s'][:, None]
    dy = corners[None, :, 1] / p['s'][:, None]
    X = cx + p['tx'][:, None] + c_ * dx - s_ * dy
    Y = cy + p['ty'][:, None] + s_ * dx + c_ * dy
    return np.stack([X, Y], axis=-1)
