"""References of a3du_joint_bilateral_upsample (include/a3d_upsample.h), on the host in numpy:

  upsample(..., dtype=np.float64)   the definition with every real-valued operation in float64;
  upsample(..., dtype=np.float32)   the definition restated in float32 in the kernel's order: every operation rounded on
                                    its own, cells in ascending (i, j), np.exp in float32;
  literal(...)                      sum f g d / sum f g with nothing subtracted from the exponents, float64, written as
                                    plain loops (for moderate sigmas, where nothing underflows);
  tables_corner / tables_block      the two table builders, as plain scalar loops in float64.

The window centre is part of the definition AS A FLOAT32 RESULT, clamp(floor(fl(c + 1/2)), 0, g - 1): it is a discrete
choice, so the float64 reference takes the same one (an exact c + 1/2 just below an integer can round up to it)."""
import math

import numpy as np

GRID = (240, 320)


def tables_corner(gh, gw, H, W):
    """msdn: cell i stands for relative position i / gh.  (cy, cx float32, ay, ax int32)."""
    def axis(g, S):
        c = [u * g / S for u in range(S)]
        a = [min(max(math.floor(i * S / g + 0.5), 0), S - 1) for i in range(g)]
        return np.array(c, np.float64).astype(np.float32), np.array(a, np.int32)
    (cy, ay), (cx, ax) = axis(gh, H), axis(gw, W)
    return cy, cx, ay, ax


def tables_block(sp, H, W):
    """dcnf: cell R is the mean of rows [R sp, (R + 1) sp) of the 240 x 320 grid; the anchor is the middle image row of
    the rows the block covers, the later one of two."""
    def axis(G, S):
        c = [(u * G / S + 0.5) / sp - 0.5 for u in range(S)]
        a = [min(max(math.floor((r + 0.5) * sp * S / G), 0), S - 1) for r in range(G // sp)]
        return np.array(c, np.float64).astype(np.float32), np.array(a, np.int32)
    (cy, ay), (cx, ax) = axis(GRID[0], H), axis(GRID[1], W)
    return cy, cx, ay, ax


def guide_values(guide):
    """float32 guide as the kernel reads it: float32 as it is, uint8 k as fl(k / 255)."""
    guide = np.asarray(guide)
    return guide.astype(np.float32) / np.float32(255) if guide.dtype == np.uint8 else guide.astype(np.float32)


def centre(c, g):
    """clamp(floor(fl(c + 1/2)), 0, g - 1) on a float32 table; a NaN goes to 0."""
    with np.errstate(invalid='ignore'):
        q = np.floor(np.asarray(c, np.float32) + np.float32(0.5))
    q = np.where(np.isnan(q), 0, np.clip(q, 0, g - 1))
    return q.astype(np.int64)


def upsample(depth, guide, cy, cx, ay, ax, R, inv2ss, inv2sr, dtype=np.float64, e_add=0.0, shifted=True):
    """depth [n,gh,gw] float32, guide [n,H,W,3] (float32 or uint8), the four tables, inv2ss / inv2sr as the float32 the
    kernel gets -> out [n,H,W] of `dtype`.  e_add: a constant added to every exponent; shifted=False: w = exp(-e)."""
    f = dtype
    depth = np.asarray(depth, np.float32)
    g32 = guide_values(guide)
    n, gh, gw = depth.shape
    H, W = g32.shape[1:3]
    cy, cx = np.asarray(cy, np.float32), np.asarray(cx, np.float32)
    ay, ax = np.asarray(ay, np.int64), np.asarray(ax, np.int64)
    anchor_ok = ((ay >= 0) & (ay < H))[:, None] & ((ax >= 0) & (ax < W))[None, :]
    cell_rgb = g32[:, np.clip(ay, 0, H - 1)[:, None], np.clip(ax, 0, W - 1)[None, :], :].astype(f)      # [n,gh,gw,3]
    gp = g32.astype(f)
    q0y, q0x = centre(cy, gh), centre(cx, gw)
    ss, sr = f(np.float32(inv2ss)), f(np.float32(inv2sr))
    es, ds, keeps = [], [], []
    with np.errstate(all='ignore'):
        for di in range(-R, R + 1):
            for dj in range(-R, R + 1):
                i, j = (q0y + di)[:, None], (q0x + dj)[None, :]
                ingrid = (i >= 0) & (i < gh) & (j >= 0) & (j < gw)
                ic, jc = np.clip(i, 0, gh - 1), np.clip(j, 0, gw - 1)
                d = depth[:, ic, jc].astype(f)
                dy, dx = i.astype(f) - cy.astype(f)[:, None], j.astype(f) - cx.astype(f)[None, :]
                space = dy * dy + dx * dx
                diff = gp - cell_rgb[:, ic, jc, :]
                rng = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
                e = (space * ss)[None] + rng * sr
                keep = ingrid[None] & anchor_ok[ic, jc][None] & np.isfinite(d) & np.isfinite(e)
                es.append(e + f(e_add)), ds.append(d), keeps.append(keep)
        big = f(np.inf)
        e_min = np.minimum.reduce([np.where(k, e, big) for e, k in zip(es, keeps)])
        d_min = np.minimum.reduce([np.where(k, d, big) for d, k in zip(ds, keeps)])
        d_max = np.maximum.reduce([np.where(k, d, -big) for d, k in zip(ds, keeps)])
        num, den = np.zeros((n, H, W), f), np.zeros((n, H, W), f)
        for e, d, k in zip(es, ds, keeps):
            w = np.where(k, np.exp(-(e - e_min) if shifted else -e), f(0))
            num = num + np.where(k, w * np.where(k, d, f(0)), f(0))
            den = den + w
        v = np.minimum(np.maximum(num / den, d_min), d_max)
    out = np.where(e_min < big, v, f(np.nan))
    assert out.dtype == f
    return out


def literal(depth, guide, cy, cx, ay, ax, R, inv2ss, inv2sr):
    """sum f g d / sum f g over the window's cells, f = exp(-dist^2 inv2ss), g = exp(-|colour difference|^2 inv2sr), in
    float64, one pixel and one cell at a time; finite depths, anchors inside the image."""
    depth, g = np.asarray(depth, np.float64), guide_values(guide).astype(np.float64)
    n, gh, gw = depth.shape
    H, W = g.shape[1:3]
    out = np.zeros((n, H, W))
    for b in range(n):
        for y in range(H):
            for x in range(W):
                qy, qx = int(centre(cy[y:y + 1], gh)[0]), int(centre(cx[x:x + 1], gw)[0])
                num = den = 0.0
                for i in range(max(qy - R, 0), min(qy + R, gh - 1) + 1):
                    for j in range(max(qx - R, 0), min(qx + R, gw - 1) + 1):
                        fs = math.exp(-((i - float(cy[y])) ** 2 + (j - float(cx[x])) ** 2) * float(np.float32(inv2ss)))
                        gr = math.exp(-float(((g[b, y, x] - g[b, ay[i], ax[j]]) ** 2).sum()) * float(np.float32(inv2sr)))
                        num += fs * gr * depth[b, i, j]
                        den += fs * gr
                out[b, y, x] = num / den
    return out


def window_range(depth, cy, cx, R):
    """(lo, hi) [n,H,W] float32: the smallest and largest finite depth among the grid cells of every pixel's window
    (+inf / -inf where it holds none)."""
    depth = np.asarray(depth, np.float32)
    n, gh, gw = depth.shape
    q0y, q0x = centre(cy, gh), centre(cx, gw)
    lo = np.full((n, len(q0y), len(q0x)), np.inf, np.float32)
    hi = -lo
    for di in range(-R, R + 1):
        for dj in range(-R, R + 1):
            i, j = (q0y + di)[:, None], (q0x + dj)[None, :]
            d = depth[:, np.clip(i, 0, gh - 1), np.clip(j, 0, gw - 1)]
            ok = ((i >= 0) & (i < gh) & (j >= 0) & (j < gw))[None] & np.isfinite(d)
            lo, hi = np.where(ok, np.minimum(lo, d), lo), np.where(ok, np.maximum(hi, d), hi)
    return lo, hi


def inv2(sigma):
    """1 / (2 sigma^2) as the float32 the launch gets; inf -> 0."""
    return np.float32(0.0 if sigma == float('inf') else 1.0 / (2.0 * sigma * sigma))
