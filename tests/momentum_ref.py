"""SGD with momentum as include/a3d_optim.h states it (TensorFlow 1.3's ApplyMomentum without Nesterov), on the host.  A plain
helper module, no GPU and no torch: tests/test_momentum_cpu.py pins it against torch.optim.SGD.

    g'     = grad_scale == 1 ? g : g * grad_scale
    accum' = accum * momentum + g'
    var'   = var - lr * accum'

step() is the rule in numpy float32: `acc * mu + g` and `var - lr * acc` as numpy writes them are two roundings each (numpy
never fuses a multiply with an add), which is what the kernels do with -ffp-contract=off.  step64() is the same rule in float64,
for operands on which every float32 operation is exact."""
import numpy as np


def step(var, accum, g, lr, momentum, grad_scale=1.0):
    """(var', accum') as float32 arrays; the arguments are not changed."""
    var, accum, g = (np.asarray(a, np.float32) for a in (var, accum, g))
    lr, mu, s = np.float32(lr), np.float32(momentum), np.float32(grad_scale)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        if s != np.float32(1.0):
            g = g * s
        accum = accum * mu + g
        var = var - lr * accum
    return var, accum


def step64(var, accum, g, lr, momentum, grad_scale=1.0):
    """The same rule in float64."""
    var, accum, g = (np.asarray(a, np.float64) for a in (var, accum, g))
    accum = accum * float(momentum) + g * float(grad_scale)
    return var - float(lr) * accum, accum
