"""Host references of superpixel pooling (include/a3d_fcsp.h) and of DCNF's fully convolutional unary (--unary fcsp).

TEST INFRASTRUCTURE ONLY.  Three statements of the pooling: the integer counts from the tables; float64, both directions,
as two small matrix products; and float32 in the order the header gives the kernels (cells ascending, zero weights
skipped, every operation rounded on its own, one division), which the GPU tests hold the kernels to bit for bit.  The
unary stack at any image size is built from oracle.tf13_ops, with a pixel-to-cell map derived here on its own (receptive
fields pushed through the layers, nearest centre by comparison), not by models.fcsp_maps' formula."""
import numpy as np

from oracle import dcnf as OD
from oracle import tf13_ops as T

U = 2.0 ** -24          # unit roundoff of float32


def counts(table, sp, cells):
    """cy [R, i] = #{ y in [R sp, (R + 1) sp) : table[y] == i }, int64; entries outside [0, cells) count nowhere."""
    table = np.asarray(table, np.int64)
    assert table.ndim == 1 and table.size % sp == 0
    out = np.zeros((table.size // sp, cells), np.int64)
    for y, v in enumerate(table):
        if 0 <= v < cells:
            out[y // sp, v] += 1
    return out


def pool_fwd64(feat, ymap, xmap, sp):
    """feat [n,h,w,C] -> [n,S,C] float64 (finite data: 0 * x is taken as 0)."""
    n, h, w, C = feat.shape
    cy, cx = counts(ymap, sp, h).astype(np.float64), counts(xmap, sp, w).astype(np.float64)
    out = np.einsum('Ri,Qj,bijc->bRQc', cy, cx, feat.astype(np.float64)) / float(sp * sp)
    return out.reshape(n, -1, C)


def pool_bwd64(dpooled, ymap, xmap, sp, h, w):
    """dpooled [n,S,C] -> [n,h,w,C] float64, the transpose of pool_fwd64."""
    n, S, C = dpooled.shape
    cy, cx = counts(ymap, sp, h).astype(np.float64), counts(xmap, sp, w).astype(np.float64)
    d = dpooled.astype(np.float64).reshape(n, cy.shape[0], cx.shape[0], C)
    return np.einsum('Ri,Qj,bRQc->bijc', cy, cx, d) / float(sp * sp)


def pool_fwd32(feat, ymap, xmap, sp):
    """The forward kernel's arithmetic: float32, the sum started at +0, cells in ascending (i, j), zero weights skipped."""
    feat = np.asarray(feat, np.float32)
    n, h, w, C = feat.shape
    cy, cx = counts(ymap, sp, h), counts(xmap, sp, w)
    out = np.empty((n, cy.shape[0], cx.shape[0], C), np.float32)
    div = np.float32(sp * sp)
    with np.errstate(invalid='ignore', over='ignore'):
        for R in range(cy.shape[0]):
            rows = np.flatnonzero(cy[R])
            for Q in range(cx.shape[0]):
                cols = np.flatnonzero(cx[Q])
                acc = np.zeros((n, C), np.float32)
                for i in rows:
                    for j in cols:
                        acc = acc + np.float32(cy[R, i] * cx[Q, j]) * feat[:, i, j, :]
                out[:, R, Q] = acc / div
    return out.reshape(n, -1, C)


def pool_bwd32(dpooled, ymap, xmap, sp, h, w):
    """The backward kernel's arithmetic: float32, superpixels ascending, zero weights skipped, +0 where nothing maps."""
    dpooled = np.asarray(dpooled, np.float32)
    n, S, C = dpooled.shape
    cy, cx = counts(ymap, sp, h), counts(xmap, sp, w)
    SC = cx.shape[0]
    out = np.empty((n, h, w, C), np.float32)
    div = np.float32(sp * sp)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(h):
            srows = np.flatnonzero(cy[:, i])
            for j in range(w):
                scols = np.flatnonzero(cx[:, j])
                acc = np.zeros((n, C), np.float32)
                for R in srows:
                    for Q in scols:
                        acc = acc + np.float32(cy[R, i] * cx[Q, j]) * dpooled[:, R * SC + Q, :]
                out[:, i, j] = acc / div
    return out


def fwd_terms_abs(feat, ymap, xmap, sp):
    """sum |terms| / (sp sp) of every forward output, float64: what the float32 error bound is relative to."""
    return pool_fwd64(np.abs(np.asarray(feat, np.float64)), ymap, xmap, sp)


def window_cells(ymap, xmap, sp, h, w):
    """The largest number of cells with a positive weight in one superpixel, and of superpixels on one cell."""
    cy, cx = counts(ymap, sp, h) > 0, counts(xmap, sp, w) > 0
    fwd = int(cy.sum(1).max() * cx.sum(1).max())
    bwd = int(cy.sum(0).max() * cx.sum(0).max())
    return fwd, bwd


# ----------------------------------------------------------------------------------------------------------------------
# the unary stack over a whole image
# ----------------------------------------------------------------------------------------------------------------------
def map_size(H, W):
    h, w = H, W
    for n, ks in OD.CONVS:
        h, w = h - ks[0] + 1, w - ks[1] + 1
        if n in OD.POOL_AFTER:
            h, w = h // 2, w // 2
    return h, w


def receptive_field(cell):
    """[lo, hi] of the image rows that cell `cell` of the last pooled map sees, pushed back through the layers."""
    lo = hi = cell
    for n, ks in reversed(OD.CONVS):
        if n in OD.POOL_AFTER:
            lo, hi = 2 * lo, 2 * hi + 1
        hi = hi + ks[0] - 1
    return lo, hi


def centre_table(size, cells):
    """Pixel -> the cell whose receptive-field centre is nearest (the lower cell on a tie, of which there are none)."""
    centres = np.array([sum(receptive_field(i)) / 2.0 for i in range(cells)])
    return np.abs(np.arange(size)[:, None] - centres[None, :]).argmin(axis=1).astype(np.int32)


def param_shapes():
    s = OD.param_shapes()
    s[OD.PREFIX + 'dense/kernel'] = (256, 128)
    return s


def init_params(seed=3000, dtype=np.float32):
    """The draw of models.DCNFUnaryFCSP: oracle.dcnf.init_params' stream and order with dense/kernel [256,128]."""
    rng = np.random.default_rng(seed)
    return {n: T.glorot_uniform(rng, s, dtype) if n.endswith('/kernel') else np.zeros(s, dtype)
            for n, s in param_shapes().items()}


def unary_forward(p, resized, sp):
    """resized [B,H,W,3] -> dict of activations; 'pooled' [B*S,256], 'z' [B*S,1]."""
    a = {'x': resized}
    t = resized
    for n, _ in OD.CONVS:
        t = T.conv2d_fwd(t, p[OD.PREFIX + n + '/kernel'], p[OD.PREFIX + n + '/bias'], 1, 'VALID', True)
        a[n] = t
        if n in OD.POOL_AFTER:
            t = T.maxpool2x2_fwd(t)
            a[n + '/pool'] = t
    B, H, W, _ = resized.shape
    h, w = t.shape[1:3]
    assert (h, w) == map_size(H, W)
    ymap, xmap = centre_table(H, h), centre_table(W, w)
    t = pool_fwd64(t, ymap, xmap, sp).astype(resized.dtype).reshape(-1, t.shape[-1])
    a['pooled'] = t
    for n, _, act in OD.DENSES:
        t = T.dense_fwd(t, p[OD.PREFIX + n + '/kernel'], p[OD.PREFIX + n + '/bias'], act)
        a[n] = t
    a['z'] = t
    return a


def unary_backward(p, a, dz, sp):
    """Gradients of sum(z * dz) wrt every unary variable from the activations `a` (dz [B*S,1]); also returns the
    gradient of 'pooled' and of 'conv2d_4/pool' under those names with a 'd:' prefix."""
    g = {}
    d = dz
    for (n, _, act), xin in reversed(list(zip(OD.DENSES, ['pooled', 'dense', 'dense_1']))):
        y = a[n]
        if act == 'relu':
            d = T.relu_grad(d, y)
        elif act == 'sigmoid':
            d = d * y * (1 - y)
        d, g[OD.PREFIX + n + '/kernel'], g[OD.PREFIX + n + '/bias'] = T.dense_bwd(a[xin], p[OD.PREFIX + n + '/kernel'], d)
    g['d:pooled'] = d
    B, H, W, _ = a['x'].shape
    _, h, w, C = a['conv2d_4/pool'].shape
    d = pool_bwd64(d.reshape(B, -1, C), centre_table(H, h), centre_table(W, w), sp, h, w).astype(dz.dtype)
    g['d:conv2d_4/pool'] = d
    prev_out = {'conv2d': 'x', 'conv2d_1': 'conv2d/pool', 'conv2d_2': 'conv2d_1/pool', 'conv2d_3': 'conv2d_2',
                'conv2d_4': 'conv2d_3'}
    for n, ks in reversed(OD.CONVS):
        if n in OD.POOL_AFTER:
            d = T.maxpool2x2_bwd(a[n], d)
        dzc = T.relu_grad(d, a[n])
        x = a[prev_out[n]]
        g[OD.PREFIX + n + '/kernel'], g[OD.PREFIX + n + '/bias'] = T.conv2d_bwd_filter(x, dzc, ks, 1, 'VALID')
        if n != 'conv2d':
            d = T.conv2d_bwd_data(dzc, p[OD.PREFIX + n + '/kernel'], x.shape, 1, 'VALID')
    return g
