"""Gradient clipping by global norm as include/a3d_clip.h states it, on the host.  A plain helper module, no GPU and no torch:
tests/test_clip_cpu.py pins it against torch.nn.utils.clip_grad_norm_.

    S = sum of (double)g[i] * (double)g[i]          n = |gs| * sqrt(S)
    skip iff S is not finite: scale = 0
    otherwise scale = (float)((double)gs * C / n) if n > C, else gs

and the optimizer rules run with that scale: momentum through tests/momentum_ref.py, the two descents restated here in numpy
float32 (two roundings where the kernels, built with -ffp-contract=off, round twice).  ApplyAdam has no restatement of its own
here: the GPU tests hold its _ctl form to a3d_adam_apply_tf1_flag, which tests/test_gpu_pointwise.py holds to the oracle's."""
import collections

import numpy as np

import momentum_ref as MR

Clip = collections.namedtuple('Clip', 'sumsq norm scale skip')      # float64, float32, float32, 0 / 1


def sumsq(g):
    """S in float64.  Each term is exact (24-bit significands); the sum's order is numpy's, any order is within 2^-26 relative
    for up to 2^27 non-negative terms, and exact where S < 2^53 on integer-valued g."""
    g = np.asarray(g, np.float32).astype(np.float64).ravel()
    with np.errstate(invalid='ignore', over='ignore'):
        return float(np.sum(g * g))


def clip(g, grad_scale, clip_norm, S=None):
    """The definition on gradient g (or on a given S)."""
    S = sumsq(g) if S is None else float(S)
    gs, C = np.float32(grad_scale), np.float32(clip_norm)
    with np.errstate(invalid='ignore', over='ignore'):
        n = np.abs(np.float64(gs)) * np.sqrt(np.float64(S))
        if not np.isfinite(S):
            return Clip(S, np.float32(n), np.float32(0), 1)
        scale = np.float32(np.float64(gs) * np.float64(C) / n) if n > np.float64(C) else gs
        return Clip(S, np.float32(n), scale, 0)


def momentum(var, accum, g, lr, mu, c):
    """(var', accum') under Clip c: untouched on a skip."""
    if c.skip:
        return np.array(var, np.float32), np.array(accum, np.float32)
    return MR.step(var, accum, g, lr, mu, c.scale)


def sgd(var, g, lr, c, floor=None):
    """var' of gradient descent at fl32(lr * scale) under Clip c, floored where a floor is given; untouched on a skip."""
    var, g = np.asarray(var, np.float32), np.asarray(g, np.float32)
    if c.skip:
        return var.copy()
    with np.errstate(all='ignore'):
        out = var - (np.float32(lr) * np.float32(c.scale)) * g
        if floor is not None:
            out = np.where(out < np.float32(floor), np.float32(floor), out)
    return out
