"""NON-REFERENCE: parameter draws of the train-time augmentation of Eigen et al. 2014, section 3.4 (host side, numpy only).

One row of 12 float32 per image, in the layout a3d_warp_bilinear_pair reads (include/a3d.h, A3D_WARP_STRIDE):

    m00 m01 m02 m10 m11 m12   g0 g1 g2 g3   gd   0

The six m are the map  p' = c + t + R(r) diag(+-1, 1) (p - c) / s  about the image centre c = ((w-1)/2, (h-1)/2), a
transformation of SOURCE space in source pixels: the same numbers serve the image and the depth map, whose output grids
differ.  g0..g2 are the colour gains, g3 = 1, gd = 1/s (the paper divides depths by s).

Draws per image, in float64, rounded once to float32:
  r   rotation, uniform in +-rotate_deg
  s   scale, uniform in [max(s_lo, s_fit(r)), s_hi] with
      s_fit(r) = max(1, ((w-1) cos|r| + (h-1) sin|r|) / (w-1), ((w-1) sin|r| + (h-1) cos|r|) / (h-1)):
      the rotated window [0, w-1] x [0, h-1] / s then lies inside the stored image, so no pixel and no depth is invented
      (r = 5 degrees at 480 x 640: s_fit = 1.11; where s_fit exceeds s_hi, s = s_fit)
  t   translation, uniform over the slack that window leaves on each axis (translate=False: 0)
  flip with probability `flip`; three colour gains uniform in `color`

The draw is a pure function of (seed, rank, step): a counter-based Philox4x64 generator with key (seed, rank) and the step
in the highest counter word, so different steps read disjoint stretches of one stream and nothing is carried from step to
step.  A run resumed at step k draws what an uninterrupted run drew at k.  Every image consumes eight uniforms whatever
the settings, so switching one transformation off leaves the others' draws where they were.
"""
import dataclasses

import numpy as np

STRIDE = 12                          # A3D_WARP_STRIDE (include/a3d.h)
_DRAWS = 8                           # r, s, tx, ty, flip, g0, g1, g2


@dataclasses.dataclass(frozen=True)
class Eigen2014:
    scale: tuple = (1.0, 1.5)
    rotate_deg: float = 5.0
    color: tuple = (0.8, 1.2)
    flip: float = 0.5
    translate: bool = True


def s_fit(r, h, w):
    """The smallest scale at which the window rotated by r (radians) stays inside an h x w image."""
    c, s = np.cos(np.abs(r)), np.sin(np.abs(r))
    W, H = max(w - 1, 1), max(h - 1, 1)
    return np.maximum(1.0, np.maximum(((w - 1) * c + (h - 1) * s) / W, ((w - 1) * s + (h - 1) * c) / H))


def draw(cfg, seed, rank, step, n, h, w):
    """The float64 parameters of n images: dict of arrays r (radians), s, tx, ty, flip (+-1), gains [n, 3]."""
    if min(seed, rank, step) < 0 or n <= 0 or h <= 0 or w <= 0:
        raise ValueError(f'augment.draw: seed {seed}, rank {rank}, step {step}, n {n}, h {h}, w {w}')
    gen = np.random.Generator(np.random.Philox(key=[int(seed), int(rank)], counter=[0, 0, 0, int(step)]))
    u = gen.random((n, _DRAWS))
    r = np.deg2rad(cfg.rotate_deg) * (2.0 * u[:, 0] - 1.0)
    lo = np.maximum(cfg.scale[0], s_fit(r, h, w))
    hi = np.maximum(cfg.scale[1], lo)
    s = lo + (hi - lo) * u[:, 1]
    a, b = (w - 1) / 2.0 / s, (h - 1) / 2.0 / s
    c_, s_ = np.cos(np.abs(r)), np.sin(np.abs(r))
    slack_x = np.maximum((w - 1) / 2.0 - (a * c_ + b * s_), 0.0)
    slack_y = np.maximum((h - 1) / 2.0 - (a * s_ + b * c_), 0.0)
    on = 1.0 if cfg.translate else 0.0
    tx = on * slack_x * (2.0 * u[:, 2] - 1.0)
    ty = on * slack_y * (2.0 * u[:, 3] - 1.0)
    flip = np.where(u[:, 4] < cfg.flip, -1.0, 1.0)
    gains = cfg.color[0] + (cfg.color[1] - cfg.color[0]) * u[:, 5:8]
    return dict(r=r, s=s, tx=tx, ty=ty, flip=flip, gains=gains)


def assemble(p, h, w):
    """draw()'s parameters as the float32 [n, 12] table."""
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    c_, s_ = np.cos(p['r']), np.sin(p['r'])
    m00, m01 = p['flip'] * c_ / p['s'], -s_ / p['s'] + 0.0          # + 0.0: no negative zero in the identity row
    m10, m11 = p['flip'] * s_ / p['s'] + 0.0, c_ / p['s']
    t = np.zeros((len(p['s']), STRIDE), np.float64)
    t[:, 0], t[:, 1], t[:, 2] = m00, m01, cx + p['tx'] - (m00 * cx + m01 * cy)
    t[:, 3], t[:, 4], t[:, 5] = m10, m11, cy + p['ty'] - (m10 * cx + m11 * cy)
    t[:, 6:9] = p['gains']
    t[:, 9] = 1.0
    t[:, 10] = 1.0 / p['s']
    return t.astype(np.float32)


def table(cfg, seed, rank, step, n, h, w, out=None):
    """float32 [n, 12] for the batch a replica of `rank` consumes at global step `step`; written into `out` when given."""
    t = assemble(draw(cfg, seed, rank, step, n, h, w), h, w)
    if out is None:
        return t
    out[...] = t
    return out


def identity(n):
    t = np.zeros((n, STRIDE), np.float32)
    t[:, [0, 4, 6, 7, 8, 9, 10]] = 1.0
    return t
