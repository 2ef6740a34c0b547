"""Model plugins — the surface of the reference's ``src/models.py``: module attributes ``msdn`` and ``dcnf`` that
the driver looks up with ``getattr(models, args.model)`` (src/ann3depth.py:143) and calls as
``model(inputs, targets)`` (src/ann3depth.py:145, src/models.py:179,277) to obtain one train op, executed once per
step by the driver loop (src/ann3depth.py:126-127).

Underneath there is no graph and no autograd: a replica owns flat HBM buffers (weights / gradients / Adam slots per
optimizer group, activations) and ``step()`` enqueues the fixed sequence of HIP kernels of forward, backward and
optimizer on the current stream.  Variable names are the reference's TF variable names.
"""
import collections
import contextlib
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib, augment as augment_, ops
from ._lib import ConvDesc
from .feed import DeviceFeed

NET_H, NET_W = 228, 304          # src/models.py:282
OUT_H, OUT_W = 55, 74            # src/models.py:283
SAMPLES_COARSE = 2000000         # src/models.py:302
SAMPLES_FINE = 1500000           # src/models.py:303

ConvSpec = collections.namedtuple('ConvSpec', 'name cin cout k stride padding relu')

MSDN_CONVS = [  # src/models.py:211-223,241-251
    ConvSpec('coarse/conv/conv2d_0', 3, 96, 11, 4, 'VALID', True),
    ConvSpec('coarse/conv/conv2d_1', 96, 256, 5, 1, 'SAME', True),
    ConvSpec('coarse/conv/conv2d_2', 256, 384, 3, 1, 'SAME', True),
    ConvSpec('coarse/conv/conv2d_3', 384, 384, 3, 1, 'SAME', True),
    ConvSpec('coarse/conv/conv2d_4', 384, 256, 3, 2, 'VALID', True),
    ConvSpec('fine/first/conv2d', 3, 63, 9, 2, 'VALID', True),
    ConvSpec('fine/second/conv2d', 64, 64, 5, 1, 'SAME', True),
    ConvSpec('fine/third', 64, 1, 5, 1, 'SAME', False),
]
MSDN_DENSES = [('coarse/dense/dense_0', 12288, 4096), ('coarse/dense/dense_1', 4096, OUT_H * OUT_W)]

# optimizer name -> (learning rate, variable scopes)   src/models.py:318-338
MSDN_OPTIMIZERS = collections.OrderedDict([
    ('CoarseConv', (0.001, ['coarse/conv'])),
    ('CoarseDense', (0.1, ['coarse/dense'])),
    ('FineA', (0.001, ['fine/first', 'fine/third'])),
    ('FineB', (0.01, ['fine/second'])),
])


def glorot_uniform(rng, shape):
    """tf.layers default kernel_initializer (glorot_uniform): limit = sqrt(6/(fan_in+fan_out)), fans include k*k."""
    if len(shape) == 2:
        fan_in, fan_out = shape
    else:
        rf = int(np.prod(shape[:-2]))
        fan_in, fan_out = shape[-2] * rf, shape[-1] * rf
    limit = math.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-limit, limit, size=shape).astype(np.float32)


def phase_of(global_step, batchsize):
    """src/models.py:301-305,348-365: 1 = coarse, 2 = fine, 3 = only global_step += 1."""
    steps_coarse = SAMPLES_COARSE // batchsize
    steps_fine = SAMPLES_FINE // batchsize
    if global_step < steps_coarse:
        return 1
    if global_step < steps_coarse + steps_fine:
        return 2
    return 3


class ParamGroup:
    """All variables of one tf.train.AdamOptimizer instance in ONE flat buffer (plus gradient and the m / v slots),
    so the optimizer is a single streaming kernel and the data-parallel all-reduce a single bucket."""
    ALIGN = 64   # elements; keeps every tensor 256-byte aligned for 16-byte vector loads
    optimizer = 'adam'      # a group built with 'momentum' carries its own, and its momentum

    clip_norm = None        # a group built with a clip norm carries its own, a control block and a workspace

    def __init__(self, name, lr, shapes, device, beta1=0.9, beta2=1.0, eps=1e-8, slots=True, multiple=1, optimizer='adam',
                 momentum=0.9, clip_norm=None):
        """multiple: the flat length is padded (with zeros that stay zeros) to a multiple of multiple * ALIGN elements, so
        that `multiple` data-parallel ranks can cut any bucket of it into equal, 256-byte-aligned slices.
        optimizer 'momentum' (NON-REFERENCE): tf.train.MomentumOptimizer(lr, momentum) without Nesterov (ops.momentum_apply):
        `m` is its accumulator, there is no `v`, and the beta powers go unused.
        clip_norm (NON-REFERENCE, include/a3d_clip.h): every apply* becomes two launches on the same stream, the norm of the
        gradient it is about to apply (ops.grad_norm_scale into self.ctl) and the rule with its scale read from there
        (ops.*_ctl): the gradient bounded by clip_norm, a step with a non-finite gradient skipped.  The beta powers advance
        on a skipped step too: the host does not know.  None: today's launches."""
        self.name, self.lr, self.beta1, self.beta2, self.eps = name, lr, beta1, beta2, eps
        if optimizer == 'momentum':
            self.optimizer, self.momentum = optimizer, momentum
        self.offsets = collections.OrderedDict()
        off = 0
        for n, shp in shapes.items():
            self.offsets[n] = (off, tuple(shp))
            off += -(-int(np.prod(shp)) // self.ALIGN) * self.ALIGN
        off = -(-off // (multiple * self.ALIGN)) * (multiple * self.ALIGN)
        self.count = off
        self.var = torch.zeros(off, device=device)
        self.grad = torch.zeros(off, device=device)
        self.m = torch.zeros(off, device=device) if slots else None      # slots=False: plain gradient descent
        self.v = torch.zeros(off, device=device) if slots and optimizer != 'momentum' else None
        # beta powers are host scalars, updated after each apply like AdamOptimizer._finish
        self.beta1_power = np.float32(beta1)
        self.beta2_power = np.float32(beta2)
        if clip_norm is not None:
            self.clip_norm = check_clip_norm(clip_norm)
            self.ctl = ops.clip_ctl(device)
            self.ws = ops.grad_norm_ws(off, device)

    def view(self, buf, name):
        off, shp = self.offsets[name]
        return buf[off:off + int(np.prod(shp))].view(shp)

    def apply(self, grad_scale=1.0):
        self.apply_slice(0, self.count, grad_scale)
        self.advance()

    def apply_slice(self, a, b, grad_scale=1.0, poisoned=None):
        """The rule on elements [a, b) only (a data-parallel rank's slice of a reduce-scattered bucket; apply(): all of them);
        the caller advances the beta powers once per step with advance().  Under clip_norm the norm is that of the elements
        applied: a clipped group is meant to be applied whole."""
        whole = a == 0 and b == self.count
        var, m, v, g = (t if whole or t is None else t[a:b] for t in (self.var, self.m, self.v, self.grad))
        if self.clip_norm is not None:
            ops.grad_norm_scale(g, grad_scale, self.clip_norm, self.ctl, self.ws)
            if self.optimizer == 'momentum':
                ops.momentum_apply_ctl(var, m, g, self.lr, self.momentum, self.ctl)
            else:
                ops.adam_apply_tf1_ctl(var, m, v, g, self.lr, self.beta1, self.beta2, self.eps, float(self.beta1_power),
                                       float(self.beta2_power), self.ctl, poisoned=poisoned)
        elif self.optimizer == 'momentum':       # no poison flag: nothing of this rule is sharded
            ops.momentum_apply(var, m, g, self.lr, self.momentum, grad_scale)
        else:
            ops.adam_apply_tf1(var, m, v, g, self.lr, self.beta1, self.beta2, self.eps, float(self.beta1_power),
                               float(self.beta2_power), grad_scale, poisoned=poisoned)

    def frozen(self):
        """True for the optimizer the reference builds, AdamOptimizer(rate, 0.9, beta2 = 1): alpha = 0, only m moves."""
        return self.optimizer == 'adam' and self.beta2 == 1.0 and float(self.beta2_power) == 1.0

    def advance(self):
        """The beta-power bookkeeping of one ApplyAdam whose tensor work was fused elsewhere (dense_bwd_filter_adam_tf1).
        Momentum keeps no such scalar."""
        if self.optimizer == 'momentum':
            return
        self.beta1_power = self.beta1_power * np.float32(self.beta1)
        self.beta2_power = self.beta2_power * np.float32(self.beta2)

    def apply_sgd(self, grad_scale=1.0, floor=None):
        """tf.train.GradientDescentOptimizer(lr): var -= lr * grad_scale * g; floor (NON-REFERENCE): then no element below it
        (ops.sgd_apply_floor).  Under clip_norm the rate is fl32(lr * scale), scale from the norm launch."""
        if self.clip_norm is not None:
            ops.grad_norm_scale(self.grad, grad_scale, self.clip_norm, self.ctl, self.ws)
            ops.sgd_apply_ctl(self.var, self.grad, self.lr, self.ctl, floor=floor)
        elif floor is None:
            ops.sgd_apply(self.var, self.grad, self.lr * grad_scale)
        else:
            ops.sgd_apply_floor(self.var, self.grad, self.lr * grad_scale, floor)

    def clip_scalars(self, rec):
        """This group's summary scalars of the last applied step into rec (one copy of the control block; the caller has
        synchronised or does not mind waiting)."""
        st = ops.clip_read(self.ctl)
        rec[f'optimizers/GradNorm/{self.name}'] = float(st.norm)
        rec[f'optimizers/ClipScale/{self.name}'] = float(st.scale)
        rec[f'optimizers/SkippedSteps/{self.name}'] = st.skipped


def check_clip_norm(clip_norm):
    """None, or the bound on every optimizer group's gradient norm as a float: a number > 0, inf allowed (measure and skip, never
    clip); ValueError for anything else, NaN included."""
    if clip_norm is None:
        return None
    c = float(clip_norm)
    if not c > 0:
        raise ValueError(f'clip_norm {clip_norm!r}: a number > 0 (inf: measure the norms and skip non-finite steps, never clip)')
    return c


def check_valid_range(valid_range):
    """None, or (min_depth, max_depth) as two floats; ValueError unless they are two numbers in that order."""
    if valid_range is None:
        return None
    lo, hi = (float(v) for v in valid_range)
    if not lo <= hi:
        raise ValueError(f'valid_range {valid_range!r}: (min_depth, max_depth) with min_depth <= max_depth')
    return lo, hi


def check_rows(who, n, B, what, *have, ready=True, tail=''):
    """A replica at batch B reads rows [0, n) of `what` (a description of tensors holding `have` rows each): ValueError
    unless 0 < n <= B and every tensor has them (and, for a call that reuses an earlier one's results, they are ready)."""
    if not (ready and 0 < n <= min(B, *have)):
        raise ValueError(f'{who}: n = {n} rows of {what}, replica batch {B}{tail}')


class Replica:
    """What the two models' replicas do alike beyond their interface (state_dict() and self.global_step are each one's own)."""

    def tf_variables(self):
        """name -> ndarray in TensorFlow's naming, for tfckpt.write_bundle (a state's 'optimizer' string is not a variable)."""
        out = {}
        for k, v in self.state_dict().items():
            if k == 'optimizer':
                continue
            a = v.detach().cpu().numpy()
            out[k] = a.astype(np.int64) if k == 'global_step' else a.astype(np.float32)
        return out

    def _broadcast_step(self, dist, src, more=()):
        """One collective: global_step, and the host scalars `more`, from rank src as float64; returns the latter."""
        st = torch.tensor([self.global_step, *more], dtype=torch.float64, device=self.device)
        dist.broadcast(st, src)
        self.global_step = int(st[0].item())
        return [x.item() for x in st[1:]]


# The loss launches of one MSDNReplica, and what else differs between the objectives: the floats a forward launch writes (the loss
# their first), the name its four-float buffers go by (loss_<name>_c / _f), the summary tags of the words behind the valid
# fraction as (word, tag), the instance attributes the objective leaves, the workspace factory, fwd(out, tgt, loss, ws) and
# bwd(out, tgt, ws, dout, dout16).  fwd and bwd hold the objective's parameters from construction on: a replica's grad_weight,
# berhu_fraction and valid_range only report them.  A new objective is one more record here.
LossLaunches = collections.namedtuple('LossLaunches', 'width name tags attrs ws fwd bwd')
MSDN_OBJECTIVES = ('silog', 'berhu', 'ssi')
MSDN_OPTIMIZER_RULES = ('adam', 'momentum')
MSDN_PHASE_GROUPS = {1: ('CoarseConv', 'CoarseDense'), 2: ('FineA', 'FineB')}      # the optimizer groups a phase's step applies


def checkpoint_optimizer(state):
    """The optimizer that wrote a checkpoint's state (a .pt state dict or the tensors of a TF bundle): 'momentum' when the state
    says so, or when it holds slots '<var>/<Group>' and not one '<var>/<Group>_1' (a bundle carries no string; TensorFlow's
    MomentumOptimizer(name=<Group>) keeps that one slot per variable, its AdamOptimizer two); otherwise 'adam'.  The slot must
    be there for EVERY model variable the state holds: a bundle with some of Adam's first slots and none of its second (a
    partial TensorFlow checkpoint, which an Adam replica restores with the absent slots at zero) is still Adam's."""
    said = state.get('optimizer')
    if isinstance(said, str):
        return said if said == 'momentum' else 'adam'
    slots = [k for k in state if any(k.endswith('/' + g) or k.endswith('/' + g + '_1') for g in MSDN_OPTIMIZERS)]
    if not slots or any(k.endswith('_1') for k in slots):
        return 'adam'
    variables = [(n, g) for g, (_, scopes) in MSDN_OPTIMIZERS.items() for n in state
                 if n.endswith(('/kernel', '/bias')) and any(n.startswith(sc + '/') for sc in scopes)]
    return 'momentum' if variables and all(n + '/' + g in state for n, g in variables) else 'adam'


def msdn_loss_launches(objective, berhu_fraction, grad_weight, masked):
    """MSDNReplica's choice among the five launch sets, made once."""
    if objective == 'ssi':                # loss, valid fraction, mean scale, mean shift (ops.ssi_loss_fwd)
        return LossLaunches(4, 'ssi', ((2, 'scale'), (3, 'shift')), {'objective': objective}, ops.ssi_ws,
                            lambda out, tgt, loss, ws: ops.ssi_loss_fwd(out, tgt, masked, loss, ws),
                            lambda out, tgt, ws, dout, d16: ops.ssi_loss_bwd(out, tgt, masked, ws, dout, d16))
    if objective == 'berhu':              # loss, valid fraction, mean threshold, quadratic share (ops.berhu_loss_fwd)
        return LossLaunches(4, 'berhu', ((2, 'threshold'), (3, 'quadratic')),
                            {'objective': objective, 'berhu_fraction': berhu_fraction}, ops.berhu_ws,
                            lambda out, tgt, loss, ws: ops.berhu_loss_fwd(out, tgt, masked, berhu_fraction, loss, ws),
                            lambda out, tgt, ws, dout, d16: ops.berhu_loss_bwd(out, tgt, masked, berhu_fraction, ws, dout, d16))
    if grad_weight > 0:                   # total, valid fraction, silog part, gradient part (ops.silog_grad_loss_fwd)
        grid = (OUT_H, OUT_W, masked, grad_weight)
        return LossLaunches(4, 'quad', ((3, 'grad'),), {}, ops.silog_grad_ws,
                            lambda out, tgt, loss, ws: ops.silog_grad_loss_fwd(out, tgt, *grid, loss, ws),
                            lambda out, tgt, ws, dout, d16: ops.silog_grad_loss_bwd(out, tgt, *grid, ws, dout, d16))
    if masked:                            # the masked loss writes the valid fraction of the target behind the loss
        return LossLaunches(2, None, (), {}, ops.silog_masked_ws, ops.silog_masked_loss_fwd, ops.silog_masked_loss_bwd)
    return LossLaunches(1, None, (), {}, ops.silog_ws, ops.silog_loss_fwd, ops.silog_loss_bwd)


class MSDNReplica(Replica):
    """One data-parallel replica of the MSDN training graph (src/models.py:203-367) on one GPU."""
    objective = 'silog'       # the reference's loss; an instance built with 'berhu' or 'ssi' carries its own (see __init__)
    optimizer = 'adam'        # the reference's optimizer; an instance built with 'momentum' carries its own, and its momentum
    lr_scale = 1.0
    clip_norm = None

    def __init__(self, batchsize, device='cuda', params=None, seed=3000, global_step=0, beta2=1.0, reducer=None,
                 precision='fp32', keep_dense_grads=True, overlap=True, valid_range=None, grad_weight=0.0,
                 objective='silog', berhu_fraction=0.2, optimizer='adam', momentum=0.9, lr_scale=1.0, clip_norm=None):
        """precision: arithmetic of the conv contractions — 'fp32' (exact, the parity default), 'bf16x3' (split
        operands on the bf16 matrix cores, ~1e-5) or 'bf16' (BASELINE config 5).  Tensors stay float32 in HBM; the
        Cin = 3 layers, the dense layers and everything element-wise always compute in fp32.
        overlap=False: everything on the current stream (the one-stream schedule the two-stream one must equal bit for bit).
        valid_range (NON-REFERENCE): (min_depth, max_depth) — the depth maps have holes.  The target is resized (or warped)
        validity-aware: an element whose taps are not all finite and in (min_depth, max_depth] becomes NaN, and both losses
        run over the finite targets only (ops.silog_masked_loss_fwd).  None: the reference's step, launch for launch.
        grad_weight (NON-REFERENCE): weight of the gradient-matching term of Eigen & Fergus 2015 (eq. 4) in both losses: the
        squared horizontal and vertical differences of the log-depth error over the 55 x 74 grid, over the pairs of finite
        targets under valid_range.  > 0: the four loss launches are ops.silog_grad_loss_fwd / _bwd.  0: today's launches.
        objective (NON-REFERENCE): 'silog', the reference's scale-invariant log loss, or 'berhu', the reverse Huber loss of
        Laina et al. 2016 on linear depth (ops.berhu_loss_fwd / _bwd), which pulls on outputs at or below zero too; its
        threshold is berhu_fraction, in (0, 1], times the largest error of each sample; or 'ssi', the least-squares
        scale-and-shift-invariant loss of Ranftl et al. 2020 on linear depth (ops.ssi_loss_fwd / _bwd): per sample the squared
        error left after the best scale and shift of the output, the objective that matches evaluate's --align affine.
        'silog': today's launches.
        optimizer (NON-REFERENCE): 'adam', the reference's AdamOptimizer(rate, 0.9, beta2), or 'momentum', the optimizer the
        rates of MSDN_OPTIMIZERS were published for (Eigen et al. 2014): tf.train.MomentumOptimizer(rate, momentum) without
        Nesterov (ops.momentum_apply).  Each group then keeps one slot, the accumulator, where Adam keeps m and v; with
        keep_dense_grads=False the dense layers' filter gradient goes from the matrix cores straight into the update
        (ops.dense_bwd_filter_momentum).  momentum in [0, 1).  lr_scale > 0 multiplies every rate under either optimizer.
        'adam' and lr_scale 1.0: today's replica, bit for bit.
        clip_norm (NON-REFERENCE, include/a3d_clip.h): a number > 0, inf allowed.  Every optimizer group's gradient is bounded
        by its own global norm (the reduced gradient's under a reducer, at grad_scale 1 / world) and a step whose gradient is
        not finite moves nothing of that group (ParamGroup).  The norm needs the whole gradient: keep_dense_grads is forced on
        and no dense launch is fused with its update; under a reducer the dense bucket is all-reduced and applied on every rank,
        as momentum's is, its norm taken in settle().  Adam's beta powers and global_step advance on a skipped step too.
        inf on one GPU: the bits of the unfused step.  None (the default): no launch, buffer or bit differs."""
        if optimizer not in MSDN_OPTIMIZER_RULES:
            raise ValueError(f"optimizer {optimizer!r}: {' or '.join(map(repr, MSDN_OPTIMIZER_RULES))}")
        momentum, lr_scale = float(momentum), float(lr_scale)
        if not 0 <= momentum < 1:
            raise ValueError(f'momentum {momentum!r}: a number in [0, 1)')
        if not (math.isfinite(lr_scale) and lr_scale > 0):
            raise ValueError(f'lr_scale {lr_scale!r}: a finite number > 0')
        if optimizer == 'momentum' and beta2 != 1.0:
            raise ValueError(f"optimizer 'momentum' with beta2 {beta2!r}: beta2 belongs to 'adam'")
        if optimizer == 'momentum':
            self.optimizer, self.momentum = optimizer, momentum
        if lr_scale != 1.0:
            self.lr_scale = lr_scale
        if clip_norm is not None:
            self.clip_norm = check_clip_norm(clip_norm)
        if objective not in MSDN_OBJECTIVES:
            raise ValueError(f"objective {objective!r}: {', '.join(map(repr, MSDN_OBJECTIVES[:-1]))} or {MSDN_OBJECTIVES[-1]!r}")
        berhu_fraction = float(berhu_fraction)
        if not 0 < berhu_fraction <= 1:
            raise ValueError(f'berhu_fraction {berhu_fraction!r}: the threshold is a fraction in (0, 1] of the largest error')
        grad_weight = float(grad_weight)
        if not grad_weight >= 0:
            raise ValueError(f'grad_weight {grad_weight!r}: the weight of the gradient-matching term is a number >= 0')
        if objective != 'silog' and grad_weight > 0:
            raise ValueError(f"objective {objective!r} with grad_weight {grad_weight!r}: the gradient-matching term is defined "
                             f'on log differences and belongs to the silog objective')
        self.grad_weight = grad_weight
        self.valid_range = check_valid_range(valid_range)
        self._loss = msdn_loss_launches(objective, berhu_fraction, grad_weight, self.valid_range is not None)
        vars(self).update(self._loss.attrs)      # under 'silog' the instance gains no attribute and no buffer
        # keep_dense_grads=False (the training driver and bench.py on one GPU): under the reference's frozen optimizer the
        # gradient of the two dense kernels (268 MB) goes straight from the matrix cores into ApplyAdam's m slot
        # (ops.dense_bwd_filter_adam_tf1) and is never written; grad('coarse/dense/...') is then stale.  A data-parallel
        # replica needs the gradient for its all-reduce and always keeps it.
        self.keep_dense_grads = keep_dense_grads or reducer is not None or batchsize > 64 or clip_norm is not None
        # 'bf16s' = BASELINE config 5 proper: bf16 arithmetic AND bf16 storage — the conv stacks' activations and their
        # gradients, and a bf16 copy of every kernel with at least 8 input channels, live in HBM as bf16; fp32 stay the
        # master weights, the Adam slots, all filter / bias gradients and split-K slabs, the resized input, the 3-channel
        # layers' filters, fine/second's output (fine/third is a single-output-channel stencil on fp32), and the
        # tensors of the dense layers' small side (x, y, dz, dx: a few MB; dense_0's 201 MB of weights are read as bf16).
        self.bf16s = precision == 'bf16s'
        self._c4_32_fresh = False
        if self.bf16s:
            precision = 'bf16'
        self.precision = precision
        self.B = B = batchsize
        self.device = torch.device(device)
        self.global_step = global_step
        self.reducer = reducer
        dev = self.device
        # Second HIP stream (overlap=False turns it off): the fine network's forward — MFMA-bound, and in the coarse phase
        # needed only for its loss — runs beside the stretch of the coarse chain that is HBM-bound (dense forward, loss,
        # dense backward + ApplyAdam, conv2d_4 backward) and is joined before the large conv backward GEMMs start.
        # Measured on one MI355X at B = 32 (round 2): coarse-phase step 3.42 -> 3.32 ms.  The two kinds of kernel share
        # CUs only as far as the register file allows (two 8-wave GEMM blocks fill a SIMD's 512 registers), so the gain
        # is a quarter of the stretch, not all of it.  The dominant bwd-filter GEMMs run after the join, alone.
        self.overlap = overlap
        # Beside the side stream, both fine-network GEMMs are launched with A3D_HINT_SHARE_CU (at most two wavefronts per
        # SIMD, so that the dense layers' weight-streaming kernels find room on every CU): 2.939 ms per step (alternating
        # runs) against 2.947 with fine/second only, 2.98 with fine/first only, 2.985 with neither.  (fine/first's
        # few-channel kernel keeps three chunks in flight per wave under the hint; with its stand-alone schedule it lost.)
        # Starting fine/first earlier (beside the coarse conv stack) or later (after the dense forward) both lose: an
        # MFMA-bound grid beside another MFMA-bound grid only takes CU slots from it.
        self._shared_desc = {}
        # the few-channel forwards' filters in the layout their kernels read, repacked when the weights change instead of on
        # every call (a3d_conv2d_fwd_prepare_filter)
        self._prep = {}
        self._alone = ()          # fine-network GEMMs of the current forward that nothing runs beside (fine phase: fine/second)
        self._deferred = None     # (all-reduce handle, group, grad scale): CoarseDense bucket still in flight, see step()
        # data-parallel replicas under the reference's frozen optimizer: the dense bucket is reduce-scattered and each
        # rank keeps the Adam `m` slot of its own slices only (dp.py); gather_state() reassembles it
        self._m_sharded = False
        # A3D_DP_DENSE=allreduce forces the exchange without aliasing buffers (all-reduce + replicated ApplyAdam, what the
        # flagged beta2 < 1 mode always uses); the default, reduce-scatter, is taken only if the backend passes the
        # reducer's own check of the in-place collectives (dp.GradReducer.inplace_ok: RCCL has not run them on this pipeline)
        self.dense_exchange = None
        if reducer is not None:
            want = os.environ.get('A3D_DP_DENSE', 'scatter')
            if want not in ('scatter', 'allreduce'):
                raise ValueError(f'A3D_DP_DENSE={want!r}: scatter or allreduce')
            # (a clipped bucket is applied whole, from its own norm: nothing of it is sharded)
            scatter = want == 'scatter' and clip_norm is None
            self.dense_exchange = 'reduce_scatter' if (scatter and reducer.inplace_ok(dev)) else 'all_reduce'
            if scatter and self.dense_exchange == 'all_reduce':
                print('MSDNReplica: in-place reduce-scatter failed its self-check on this backend; the dense bucket is '
                      'all-reduced instead', flush=True)
        self._dense_pieces = None
        self._poison = None       # device flag: a non-finite gradient reached one of this rank's slices
        self._poison_seen = []    # [(event, pinned host copy of the all-rank MAX of the flag)] of earlier steps
        # conv + ReLU + max pool in one kernel inside step(): the pre-pool activations c0, c1, f1 are never written
        # (the network being trained keeps one byte per pool window instead, see forward()).  'bf16s' fuses all three in
        # every phase, conv2d_1's pool in the LDS-DMA kernel's epilogue (argmax bytes + a bf16 MaxPoolGrad by index).
        self.fuse_pool = precision == 'fp32'
        self.side = None
        if self.overlap and dev.type == 'cuda':
            # below the main stream's queue priority: a CU slot that frees up goes to the HBM-bound kernel first
            handle = ctypes.c_void_p()
            with torch.cuda.device(dev):
                ops.check(_lib.load().a3d_stream_create(1, ctypes.byref(handle)), 'a3d_stream_create')
            self.side = torch.cuda.ExternalStream(handle.value, device=dev)
            self._side_handle = handle.value       # ExternalStream does not own it: returned in __del__
        shapes = collections.OrderedDict()
        for c in MSDN_CONVS:
            shapes[c.name + '/kernel'] = (c.k, c.k, c.cin, c.cout)
            shapes[c.name + '/bias'] = (c.cout,)
        for n, i, o in MSDN_DENSES:
            shapes[n + '/kernel'] = (i, o)
            shapes[n + '/bias'] = (o,)
        self.shapes = shapes
        self.groups = collections.OrderedDict()
        self.group_of = {}
        for gname, (lr, scopes) in MSDN_OPTIMIZERS.items():
            gshapes = collections.OrderedDict((n, s) for n, s in shapes.items()
                                              if any(n.startswith(sc + '/') for sc in scopes))
            world = reducer.world_size if (reducer is not None and gname == 'CoarseDense') else 1
            self.groups[gname] = ParamGroup(gname, lr if lr_scale == 1.0 else lr * lr_scale, gshapes, dev, beta2=beta2,
                                            multiple=world, optimizer=optimizer, momentum=momentum, clip_norm=clip_norm)
            for n in gshapes:
                self.group_of[n] = gname
        if params is None:
            rng = np.random.default_rng(seed)
            params = {n: (glorot_uniform(rng, s) if n.endswith('/kernel') else np.zeros(s, np.float32))
                      for n, s in shapes.items()}
        self.load_params(params)

        def buf(*shape):
            return torch.empty(shape, device=dev)

        def abuf(*shape):           # an activation (or activation gradient) of the conv stacks: bf16 under 'bf16s'
            return torch.empty(shape, device=dev, dtype=torch.bfloat16 if self.bf16s else torch.float32)
        self.conv = {c.name: c for c in MSDN_CONVS}
        # activations
        self.x = buf(B, NET_H, NET_W, 3)
        self.t = buf(B, OUT_H, OUT_W, 1)
        # c0 / c1 exist only where a forward writes them: never under 'bf16s' with its pools in the conv epilogues (83 MB at B = 64)
        self.c0 = None if self.bf16s else buf(B, 55, 74, 96)
        self.c1 = None if self.bf16s else buf(B, 27, 37, 256)
        self.p0 = abuf(B, 27, 37, 96); self.p1 = abuf(B, 13, 18, 256)
        self.c2 = abuf(B, 13, 18, 384); self.c3 = abuf(B, 13, 18, 384); self.c4 = abuf(B, 6, 8, 256)
        self.drop = buf(B, 4096)
        self.coarse = buf(B, OUT_H, OUT_W, 1)
        self.f1 = buf(B, 110, 148, 63) if not self.bf16s else None        # 'bf16s': never written (fused with its pool)
        self.cat = abuf(B, OUT_H, OUT_W, 64)
        self.f2 = buf(B, OUT_H, OUT_W, 64)
        self.fine = buf(B, OUT_H, OUT_W, 1)
        # what a loss launch writes: 4, 2 or 1 floats (msdn_loss_launches).  loss_coarse / loss_fine are their first, loss_pair_*
        # the first two where there are as many, loss_<name>_* all four
        width, name = self._loss.width, self._loss.name
        self.loss_out_c = buf(width); self.loss_out_f = buf(width)
        self.loss_coarse = self.loss_out_c[:1]; self.loss_fine = self.loss_out_f[:1]
        if width >= 2:
            self.loss_pair_c = self.loss_out_c[:2]; self.loss_pair_f = self.loss_out_f[:2]
        if width == 4:
            setattr(self, f'loss_{name}_c', self.loss_out_c); setattr(self, f'loss_{name}_f', self.loss_out_f)
        # window positions of the pool maxima (all MaxPoolGrad needs besides the pooled values, see forward())
        self.a0 = torch.empty((B, 27, 37, 96), dtype=torch.uint8, device=dev)
        self.a1 = torch.empty((B, 13, 18, 256), dtype=torch.uint8, device=dev)
        self.af1 = torch.empty((B, OUT_H, OUT_W, 63), dtype=torch.uint8, device=dev)
        self.pooled_fwd = None            # which network ran conv + pool fused in the last forward
        self.ws_c = self._loss.ws(B, dev); self.ws_f = self._loss.ws(B, dev)      # per-sample sums + arrival ticket + partials
        self.t_one = buf(B, 1, 1, 1) if valid_range is not None else None    # see ops.resize_bilinear_tf1_valid
        # gradients wrt pre-activations
        self.dz1 = buf(B, OUT_H * OUT_W); self.dz0 = buf(B, 4096)
        self.dc4 = abuf(B, 6, 8, 256); self.dc3 = abuf(B, 13, 18, 384); self.dc2 = abuf(B, 13, 18, 384)
        self.dp1 = abuf(B, 13, 18, 256); self.dc1 = abuf(B, 27, 37, 256)
        self.dp0 = abuf(B, 27, 37, 96); self.dc0 = None            # dc0 (50 MB at B = 32): allocated only if the unfused path runs
        # fine/third's backward writes df2 in the type fine/second's backward reads it: bf16 under 'bf16s' (round 5)
        self.dfine = buf(B, OUT_H, OUT_W, 1); self.df2 = abuf(B, OUT_H, OUT_W, 64)
        self.dcat = abuf(B, OUT_H, OUT_W, 64); self.df1 = None      # df1 (131 MB at B = 32): allocated only if the unfused path runs
        if self.bf16s:
            self.c4_32 = buf(B, 6, 8, 256)                                          # the fp32 copy of c4 dense_0's filter gradient reads
            self.dz0_16 = torch.empty((B, 4096), device=dev, dtype=torch.bfloat16)  # dense_0's bwd-data takes dz0 as bf16
            # dense_1 ([4096, 4070]: rows of 8140 bytes, not whole 16-byte pieces) on the LDS-DMA kernel too: a bf16 copy of
            # its kernel with rows of 4072 elements (the two pad columns zero, the bias padded alike).  Its master weights,
            # gradient and ApplyAdam stay fp32.
            # bf16 x / dz into the dense layers: the LDS-DMA kernel takes them as a weight stream of at most 64 rows (ring_plan,
            # igemm_plan.cc); a larger batch keeps the dense layers' small side fp32 (B = 65..383 had no kernel)
            # and dense_1 on the fp32 kernels.
            # round 5: the casts between the bf16 conv stack and the fp32 dense side (c4 -> c4_32, drop -> drop16, coarse ->
            # cat[..., 63], dz1 -> dz1_16, dz0 -> dz0_16) leave through the reductions that produce their sources
            # (a3d_second_output) instead of five 5-us launches
            self.dense_bf16_x = B <= 64
            if not self.dense_bf16_x:
                self.dc4_32 = buf(B, 6, 8, 256)
            NP = (OUT_H * OUT_W + 7) // 8 * 8
            self.w1pad = torch.zeros((4096, NP), device=dev, dtype=torch.bfloat16)
            self.b1pad = torch.zeros((1, NP), device=dev)
            self.drop16 = torch.empty((B, 4096), device=dev, dtype=torch.bfloat16)
            self.dz1_16 = torch.zeros((B, NP), device=dev, dtype=torch.bfloat16)       # (columns 4070.. stay zero)
        # descriptors
        def D(*a):
            return ops.conv_desc(*a, precision=precision)
        self.d = {
            'coarse/conv/conv2d_0': D(B, NET_H, NET_W, 3, 96, 11, 11, 4, 'VALID'),
            'coarse/conv/conv2d_1': D(B, 27, 37, 96, 256, 5, 5, 1, 'SAME'),
            'coarse/conv/conv2d_2': D(B, 13, 18, 256, 384, 3, 3, 1, 'SAME'),
            'coarse/conv/conv2d_3': D(B, 13, 18, 384, 384, 3, 3, 1, 'SAME'),
            'coarse/conv/conv2d_4': D(B, 13, 18, 384, 256, 3, 3, 2, 'VALID'),
            'fine/first/conv2d': D(B, NET_H, NET_W, 3, 63, 9, 9, 2, 'VALID'),
            'fine/second/conv2d': D(B, OUT_H, OUT_W, 64, 64, 5, 5, 1, 'SAME'),
            'fine/third': D(B, OUT_H, OUT_W, 64, 1, 5, 5, 1, 'SAME'),
        }
        # fp32: the two stride-1 3x3 layers' bwd-data through Winograd F(2x2,3x3) ('fp32w', csrc/wino.hip) from WINO_MIN_TILES
        # 2x2 tiles up; their forwards, and every layer below that, stay on the direct kernels
        self.d_wino = {}
        if precision == 'fp32' and dev.type == 'cuda':
            for n in self.WINO_LAYERS:
                d = self.d[n]
                if d.n * -(-d.ho // 2) * -(-d.wo // 2) >= self.WINO_MIN_TILES:
                    e = self.d_wino[n] = ConvDesc.from_buffer_copy(d)
                    e.precision = ops.PREC['fp32w']
        # ... and their filter gradients through the same identity (include/a3d_wino_grad.h) from WINO_GRAD_MIN_TILES tiles up
        self.wino_grad = set()
        if precision == 'fp32' and dev.type == 'cuda':
            for n in self.WINO_GRAD_LAYERS:
                d = self.d[n]
                if d.n * -(-d.ho // 2) * -(-d.wo // 2) >= self.WINO_GRAD_MIN_TILES:
                    self.wino_grad.add(n)
        # ... and the two gradients of the stride-1 5x5 layer through 1-D Winograd F(4,5) along the width (include/a3d_wino1d.h),
        # each from its own count of rows of 4-column tiles up
        self.wino1d_bwd_d, self.wino1d_bwd_f = set(), set()
        if precision == 'fp32' and dev.type == 'cuda':
            for n in self.WINO1D_LAYERS:
                d = self.d[n]
                rows = d.n * d.h * -(-d.w // 4)
                if rows >= self.WINO1D_BWD_D_MIN_ROWS:
                    self.wino1d_bwd_d.add(n)
                if rows >= self.WINO1D_BWD_F_MIN_ROWS:
                    self.wino1d_bwd_f.add(n)
        # conv -> ReLU -> pool blocks on the 3-channel image: filter gradient straight from the POOLED map's gradient (MaxPoolGrad
        # by index + ReluGrad while the kernel stages its operand): dc0 / df1 (50 / 131 MB at B = 32) are never written or read.
        # fp32 arithmetic on the fp32 image in every precision mode but 'bf16s'.
        self.d_few = {}
        if dev.type == 'cuda':
            # 'bf16s' (config 5): the same launch in bf16 arithmetic (fewch16.hip: fp32 image, bf16 pooled tensors, both operands
            # transposed into LDS); conv2d_0 there: 68 + 11 us at B = 64 against 78 + 5 + 18 for igemm_bf16 + MaxPoolGrad by index
            few_prec = 'bf16' if self.bf16s else 'fp32'
            for n, dd in (('coarse/conv/conv2d_0', ops.conv_desc(B, NET_H, NET_W, 3, 96, 11, 11, 4, 'VALID', precision=few_prec)),
                          ('fine/first/conv2d', ops.conv_desc(B, NET_H, NET_W, 3, 63, 9, 9, 2, 'VALID', precision=few_prec))):
                if ops.conv2d_bwd_filter_pooled_supported(dd):
                    self.d_few[n] = dd
        # bf16 storage: per layer, which tensors of the forward / bwd-data / bwd-filter call are bf16 (ops.STORE_*), and
        # the bf16 copies of the kernels (refreshed whenever the fp32 masters change)
        self.store = {}
        self.wcopy = {}
        if self.bf16s:
            X, W, Y = ops.STORE_X, ops.STORE_W, ops.STORE_Y
            for n in ('coarse/conv/conv2d_1', 'coarse/conv/conv2d_2', 'coarse/conv/conv2d_3', 'coarse/conv/conv2d_4'):
                self.store[n] = {'fwd': X | W | Y, 'bwd_d': X | W | Y, 'bwd_f': X | Y}
            # conv2d_0's filter gradient where the pooled launch (d_few) does not take the shape: the fp32 image and a bf16 dc0
            # through the bf16 kernel (window runs of 36 floats, 16-byte loads), 108 us against 221 us in fp32 at B = 64
            self.store['coarse/conv/conv2d_0'] = {'bwd_f': Y}
            # fine/first's filter gradient there stays fp32 (its window runs start 24 bytes apart: 8-byte loads only, which
            # the bf16 kernel does not take)
            self.d['fine/first/conv2d'].precision = ops.PREC['fp32']
            # f2 stays fp32 (fine/third is a single-output-channel stencil on fp32); df2 comes back from that layer's fused
            # backward as bf16, so fine/second's bwd-data and bwd-filter read two bf16 operands (the LDS-DMA kernel)
            self.store['fine/second/conv2d'] = {'fwd': X | W, 'bwd_d': W | X | Y, 'bwd_f': X | Y}
            # fine/first's forward runs on the bf16 pipe from a 4-channel bf16 copy of the image (8-byte pixels: window runs
            # 16 bytes apart), conv + ReLU + max pool in one launch: f1, the largest activation of the model, is never written.
            # 0.41 -> 0.10 ms at B = 64 where the layer does not train; where it trains (fine phase, round 5) the fp32
            # few-channel kernel took 0.38 ms of that phase's 1.73.
            self.x4 = torch.empty((B, NET_H, NET_W, 4), device=dev, dtype=torch.bfloat16)
            # round 5: conv2d_0's forward from the same 4-channel bf16 image (conv3.hip's bf16 form, straight from L2) instead
            # of the fp32 image through igemm_bf16's window runs
            self.w0_4 = torch.zeros((11, 11, 4, 96), device=dev)
            self.d0_4 = ops.with_storage(ops.conv_desc(B, NET_H, NET_W, 4, 96, 11, 11, 4, 'VALID', ldy=96, precision='bf16'),
                                         X | Y)
            self.w4 = torch.zeros((9, 9, 4, 63), device=dev)
            self.d4 = ops.with_storage(ops.conv_desc(B, NET_H, NET_W, 4, 63, 9, 9, 2, 'VALID', ldy=64, precision='bf16'),
                                       X | Y)
            for n in list(self.store) + ['coarse/dense/dense_0']:
                if n == 'coarse/dense/dense_0' or self.store[n].get('fwd', 0) & W:
                    self.wcopy[n] = torch.empty(self.shapes[n + '/kernel'], device=dev, dtype=torch.bfloat16)
            self.refresh_weight_copies()

    def __del__(self):
        handle, self._side_handle = getattr(self, '_side_handle', None), None
        if handle:
            try:
                torch.cuda.synchronize(self.device)
                ops.drop_workspace(handle)
                _lib.load().a3d_stream_destroy(handle)
            except Exception:          # noqa: BLE001 - interpreter shutdown: the driver reclaims the stream
                pass

    SHARE_CU = ('fine/first/conv2d', 'fine/second/conv2d')     # forwards hinted A3D_HINT_SHARE_CU beside the side stream
    # Winograd for the bwd-data of conv2d_2 / conv2d_3 (precision 'fp32' only).  Per launch, both routes timed at B = 8, 16, 32
    # on one MI355X (tools/bench_layers.py, profiles/wino_bench_layers.txt): both bwd-data launches win at each — 504 tiles
    # (B = 8) by 5-22 %, 2016 (B = 32) by 35-36 % — and nothing smaller was measured, so the threshold is the smallest count that
    # was.  Above 252: the pinned plans and records of B <= 4 (tests/golden/plan_log.json, test_make_train_drop_in) are the
    # direct kernels'.  The FORWARDS win as well (39-41 % at B = 32) and stay direct all the same: Winograd moves the coarse map
    # by 8e-7 rel-L2, and the scale-invariant log loss of an untrained network has outputs so close to zero that one of them
    # moves by 1.6 % with it; its 1/y gradient moves as much, an output that crosses zero is switched by the masked log, and the
    # Adam m slots after 25 steps differ from the direct forward's by more than their own norm.  bwd-data changes the conv
    # gradients by 7e-7 rel-L2 and nothing else (profiles/wino_outputs_vs_parent.txt).
    WINO_LAYERS = ('coarse/conv/conv2d_2', 'coarse/conv/conv2d_3')
    WINO_MIN_TILES = 504
    # The filter gradients of the same layers through the same identity (ops.conv2d_bwd_filter_wino; precision 'fp32' only).
    # tools/bench_layers.py at B = 8, 16, 32 (profiles/wino_grad_bench_layers.txt), conv2d_2 / conv2d_3, direct -> route:
    # 51.8 / 64.0 -> 45.9 / 51.3 us, 79.9 / 99.9 -> 60.5 / 73.9, 135.8 / 172.8 -> 95.1 / 124.0: both win at each, so the
    # threshold is again the smallest count measured, and B <= 4 stays direct (the pinned plans and records).  Inside the step
    # at B = 32 both win too: 2.691-2.703 -> 2.614-2.629 ms.  A filter gradient feeds only its layer's Adam m
    # slot: nothing but CoarseConv's m moves, by 3.8e-7 rel-L2 (profiles/wino_grad_outputs_vs_parent.txt).
    WINO_GRAD_LAYERS = WINO_LAYERS
    WINO_GRAD_MIN_TILES = 504
    # Where both routes are on, the layer's two gradients run as one chain of three launches (include/a3d_wino_bwd.h) with the
    # bits of the separate calls; conv2d_2's also carries conv2d_1's pool gradient.  False: the separate calls (the tests' yardstick).
    WINO_BWD_CHAIN = True

    # 1-D Winograd F(4,5) along the width for the two gradients of conv2d_1 (5x5, stride 1; precision 'fp32' only).
    # A threshold counts rows of 4-column tiles, n * h * ceil(w / 4): 270 an image.  tools/bench_layers.py conv2d_1 at B = 8, 16, 32
    # (profiles/wino1d_bench_layers.txt), direct -> route: bwd-data 105.2 -> 70.6 us, 184.9 -> 115.6, 334.5 -> 192.1; filter
    # gradient 108.3 -> 68.6, 195.0 -> 109.1, 354.8 -> 179.7.  Both win at each, so both thresholds are the smallest count measured
    # (B = 8).  Inside the step at B = 32 (profiles/wino1d_ab_step.txt): 2.583-2.586 -> 2.319-2.323 ms.  B <= 4 (1080 rows) stays
    # direct whatever is measured: the pinned plans and records (tests/golden/plan_log.json, test_make_train_drop_in) are the direct kernels'.  The
    # forward stays direct for the reason given above for conv2d_2 / conv2d_3; the two gradients reach only CoarseConv's m slots.
    WINO1D_LAYERS = ('coarse/conv/conv2d_1',)
    WINO1D_BWD_D_MIN_ROWS = 2160
    WINO1D_BWD_F_MIN_ROWS = 2160

    def _desc(self, name, which):
        """The layer's conv descriptor for 'fwd' | 'bwd_d' | 'bwd_f', with that call's storage bits."""
        d = self.d[name]
        bits = self.store.get(name, {}).get(which, 0)
        if which == 'fwd' and self.side is not None and name in self.SHARE_CU and name not in self._alone:
            # a fine-network GEMM on the side stream beside the dense layers' weight streams: leave those room on every CU
            key = (name, bits)
            if key not in self._shared_desc:
                e = ops.with_storage(d, bits)
                e.hints = ops.HINT_SHARE_CU
                self._shared_desc[key] = e
            return self._shared_desc[key]
        return ops.with_storage(d, bits) if bits else d

    def _w(self, name, which='fwd'):
        """The kernel a conv / dense call reads: the bf16 copy where this call takes one, else the fp32 master."""
        if name in self.wcopy and (name not in self.store or self.store[name][which] & ops.STORE_W):
            return self.wcopy[name]
        return self._v(name + '/kernel')

    def _prepared(self, key, desc, w, which='fwd'):
        """(descriptor, filter) for a few-channel forward or a Winograd bwd-data: the prepared copy and the descriptor that says
        so, where the launch has one."""
        if self.device.type != 'cuda':
            return desc, w
        pf = self._prep.get(key)
        if pf is None:
            pf = self._prep[key] = ops.PreparedFilter(desc, self.device, which)
            pf.source = w
            if pf.ok:
                pf.refresh(w)
        return (pf.desc_prepared, pf.buf) if pf.ok else (desc, w)

    def _refresh_prepared(self):
        for pf in self._prep.values():
            if pf.ok:
                pf.refresh(pf.source)

    def refresh_weight_copies(self):
        for n, c in self.wcopy.items():
            ops.cast_bf16(self._v(n + '/kernel'), c)
        if self.bf16s:
            self.w4[:, :, :3, :] = self._v('fine/first/conv2d/kernel')
            self.w0_4[:, :, :3, :] = self._v('coarse/conv/conv2d_0/kernel')
            n = 'coarse/dense/dense_1'
            ops.cast_rows(self._v(n + '/kernel'), self.w1pad)
            ops.cast_rows(self._v(n + '/bias').view(1, -1), self.b1pad)

    def _weights_moved(self, *groups):
        """After an ApplyAdam that can change `var` (any optimizer but the reference's frozen beta2 = 1 one): the bf16
        copies the next forward / bwd-data read must follow the fp32 masters."""
        if not all(g.frozen() for g in groups):
            if self.wcopy:
                self.refresh_weight_copies()
            self._refresh_prepared()

    # ---- variables ----
    def settle(self):
        """Finish what step() left in flight across the step boundary (the CoarseDense all-reduce and its ApplyAdam).
        Every accessor below and the next forward call it; call it yourself before touching `groups[...]` directly."""
        if self._deferred is not None:
            works, group, scale = self._deferred
            self._deferred = None
            if works and isinstance(works[0], tuple):          # reduce-scattered pieces: (handle, first, last) of my slice
                self._poll_poison()
                for work, a, b in works:
                    self.reducer.wait(work)
                    group.apply_slice(a, b, scale, poisoned=self._poison)
                group.advance()
                self._m_sharded = True
                self._watch_poison()
                return
            for work in works:
                self.reducer.wait(work)
            group.apply(scale)
            self._weights_moved(group)

    def _dense_buckets(self):
        """The CoarseDense flat buffer cut for reduce-scatter, in the order the backward completes it: (early, late) where
        `early` = [(c, count)] holds dense_1's gradient only (c = its first element rounded UP to a slice boundary) and goes
        out as soon as dense_1's bwd-filter is done, `late` = [0, c) in three pieces, complete after dense_0's."""
        if self._dense_pieces is None:
            gd = self.groups['CoarseDense']
            q = self.reducer.world_size * ParamGroup.ALIGN
            c = -(-gd.offsets['coarse/dense/dense_1/kernel'][0] // q) * q
            third = -(-(c // 3) // q) * q
            self._dense_pieces = ([(c, gd.count)], [(0, third), (third, 2 * third), (2 * third, c)])
        return self._dense_pieces

    def _my_slice(self, a, b):
        n = (b - a) // self.reducer.world_size
        return a + self.reducer.rank * n, a + (self.reducer.rank + 1) * n

    def _watch_poison(self):
        """The reference's optimizer changes a weight in exactly one case: a non-finite gradient turns it into NaN.  Under
        sharding only the slice's owner sees that; the MAX of the per-rank flags (a 4-byte all-reduce per step) tells
        everybody, read on the host two steps later (no stall), and _resync() then copies the owners' var / v slices."""
        red = self.reducer
        work = red.any(self._poison)
        red.wait(work)
        if not hasattr(self, '_poison_ring'):       # four pinned words, reused (at most two reads are ever outstanding)
            ring = torch.empty(4, dtype=torch.int32)
            self._poison_ring = (ring.pin_memory() if self.device.type == 'cuda' else ring, 0)
        ring, nxt = self._poison_ring
        self._poison_ring = (ring, (nxt + 1) % 4)
        host = ring[nxt:nxt + 1]
        host.copy_(self._poison, non_blocking=True)
        ev = None
        if self.device.type == 'cuda':
            ev = torch.cuda.Event()
            ev.record()
        self._poison_seen.append((ev, host))

    def _poll_poison(self, block=False):
        while self._poison_seen and (block or len(self._poison_seen) >= 2):
            ev, host = self._poison_seen.pop(0)
            if ev is not None:
                ev.synchronize()
            if int(host.item()):
                self._resync()

    def _resync(self):
        """Every rank takes the slice owners' var and v (and m) of the dense group; clears the poison flag."""
        gd = self.groups['CoarseDense']
        early, late = self._dense_buckets()
        for a, b in early + late:
            for buf in (gd.var, gd.v, gd.m):
                self.reducer.all_gather(buf[a:b])
        self._poison.zero_()
        self._poison_seen = []
        self._m_sharded = False

    def gather_state(self):
        """COLLECTIVE under a data-parallel reducer (every rank must call it): reassembles the sharded Adam `m` slot of the
        dense group on all ranks.  The driver calls it before the chief writes a checkpoint; a no-op otherwise."""
        self.settle()
        if self._m_sharded:
            self._poll_poison(block=True)
        if self._m_sharded:
            gd = self.groups['CoarseDense']
            early, late = self._dense_buckets()
            for a, b in early + late:
                self.reducer.all_gather(gd.m[a:b])
            self._m_sharded = False

    def load_params(self, params):
        self.settle()
        for n, shp in self.shapes.items():
            g = self.groups[self.group_of[n]]
            a = np.asarray(params[n], np.float32)
            assert a.shape == tuple(shp), (n, a.shape, shp)
            g.view(g.var, n).copy_(torch.from_numpy(np.ascontiguousarray(a)))
        if getattr(self, 'wcopy', None):
            self.refresh_weight_copies()
        if getattr(self, '_prep', None):
            self._refresh_prepared()

    def _v(self, name):
        g = self.groups[self.group_of[name]]
        return g.view(g.var, name)

    def _g(self, name):
        g = self.groups[self.group_of[name]]
        return g.view(g.grad, name)

    def var(self, name):
        self.settle()
        return self._v(name)

    def grad(self, name):
        self.settle()
        return self._g(name)

    def slot(self, name, which):
        self.gather_state()        # collective under a data-parallel reducer whose dense m slot is sharded
        g = self.groups[self.group_of[name]]
        return g.view(g.m if which == 'm' else g.v, name)

    def state_dict(self):
        """name -> tensor for every variable, Adam slot (TF slot naming '<var>/<Optimizer>[_1]') and global_step.
        Collective under a data-parallel reducer (gather_state)."""
        self.gather_state()
        sd = collections.OrderedDict()
        adam = self.optimizer == 'adam'
        for n in self.shapes:
            sd[n] = self.var(n)
            sd[n + '/' + self.group_of[n]] = self.slot(n, 'm')
            if adam:
                sd[n + '/' + self.group_of[n] + '_1'] = self.slot(n, 'v')
        for gname, g in self.groups.items() if adam else ():
            sd[gname + '/beta1_power'] = torch.tensor(float(g.beta1_power))
            sd[gname + '/beta2_power'] = torch.tensor(float(g.beta2_power))
        sd['global_step'] = torch.tensor(self.global_step, dtype=torch.int64)
        if not adam:      # '<var>/<Group>' is then the accumulator (TensorFlow's slot name under MomentumOptimizer(name=<Group>))
            sd['optimizer'] = self.optimizer
        return sd

    def _check_checkpoint_optimizer(self, state):
        wrote = checkpoint_optimizer(state)
        if wrote != self.optimizer:
            raise ValueError(f"the checkpoint was written under the {wrote!r} optimizer and this replica runs {self.optimizer!r} "
                             f"('adam' keeps two slots per variable, 'momentum' one): restore it with --optimizer {wrote}")

    def load_state_dict(self, sd):
        self._check_checkpoint_optimizer(sd)
        self.gather_state()
        adam = self.optimizer == 'adam'
        for n in self.shapes:
            self.var(n).copy_(sd[n])
            self.slot(n, 'm').copy_(sd[n + '/' + self.group_of[n]])
            if adam:
                self.slot(n, 'v').copy_(sd[n + '/' + self.group_of[n] + '_1'])
        for gname, g in self.groups.items() if adam else ():
            g.beta1_power = np.float32(sd[gname + '/beta1_power'].item())
            g.beta2_power = np.float32(sd[gname + '/beta2_power'].item())
        self.global_step = int(sd['global_step'].item())
        if self.wcopy:
            self.refresh_weight_copies()
        self._refresh_prepared()

    uses_dropout = True

    def load_tf_variables(self, tensors):
        """Restore from the tensors of a TensorFlow checkpoint (tfckpt.read_bundle): every model variable by its TF
        name; Adam slots `<var>/<Optimizer>` / `<var>/<Optimizer>_1` and `global_step` when present.
        Beta powers: `<Optimizer>/beta{1,2}_power` is THIS build's name for them (tf_variables below).  TensorFlow 1.3
        creates them as plain variables `beta1_power`, `beta1_power_1`, ... under whatever name scope apply_gradients
        ran in (for the reference: inside the tf.cond of src/models.py:340-345), so a reference checkpoint's powers are
        not looked up; they are rebuilt from global_step and the phase schedule instead — exactly, since the power is
        beta multiplied into itself once per applied step in float32 (and beta2 = 1 keeps its power at 1)."""
        missing = [n for n in self.shapes if n not in tensors]
        if missing:
            raise KeyError(f'TensorFlow checkpoint lacks {len(missing)} model variables, e.g. {missing[:3]}')
        self._check_checkpoint_optimizer(tensors)
        self.load_params(tensors)
        for n in self.shapes:
            for which, suffix in (('m', ''), ('v', '_1')) if self.optimizer == 'adam' else (('m', ''),):
                key = n + '/' + self.group_of[n] + suffix
                if key in tensors:
                    self.slot(n, which).copy_(torch.from_numpy(np.ascontiguousarray(tensors[key], np.float32)))
        if 'global_step' in tensors:
            self.global_step = int(np.asarray(tensors['global_step']).reshape(-1)[0])
        steps_coarse, steps_fine = SAMPLES_COARSE // self.B, SAMPLES_FINE // self.B
        applied = {'CoarseConv': min(self.global_step, steps_coarse), 'CoarseDense': min(self.global_step, steps_coarse),
                   'FineA': min(max(self.global_step - steps_coarse, 0), steps_fine),
                   'FineB': min(max(self.global_step - steps_coarse, 0), steps_fine)}
        for gname, g in self.groups.items():
            for attr, beta in (('beta1_power', g.beta1), ('beta2_power', g.beta2)):
                key = f'{gname}/{attr}'
                if key in tensors:
                    setattr(g, attr, np.float32(np.asarray(tensors[key]).reshape(-1)[0]))
                else:
                    power = np.float32(beta)
                    for _ in range(min(applied[gname], 4096)):       # beta^(t+1); underflows to its limit long before
                        power = power * np.float32(beta)
                    setattr(g, attr, power)

    def summary_scalars(self, out):
        """Tags as the reference's name scopes 'loss' (src/models.py:288) and 'optimizers' (:347)."""
        rec = {'loss/coarse_loss': float(out['coarse_loss']), 'loss/fine_loss': float(out['fine_loss']),
               'optimizers/Phase': out['phase']}
        if self.valid_range is not None:                 # NON-REFERENCE: share of the target pixels that hold a depth
            rec['valid_fraction'] = float(self.loss_pair_c[1])
        for name, quad in (('coarse', self.loss_out_c), ('fine', self.loss_out_f)):      # NON-REFERENCE: the objective's own words
            for word, tag in self._loss.tags:
                rec[f'loss/{name}_{tag}'] = float(quad[word])
        if self.clip_norm is not None:                   # NON-REFERENCE: the groups this phase applied
            self.settle()
            for gname in MSDN_PHASE_GROUPS.get(out['phase'], ()):
                self.groups[gname].clip_scalars(rec)
        return rec

    def summary_images(self):
        """src/models.py:292-296: (tag, batch, max_outputs)."""
        target = self.t if self.valid_range is None else torch.nan_to_num(self.t[:3], nan=0.0)    # a hole is shown as 0
        return [('summaries/Input', self.x, 3), ('summaries/Coarse', self.coarse, 3), ('summaries/Fine', self.fine, 3),
                ('summaries/Target', target, 3)]

    def broadcast_state(self, dist, src=0):
        """Non-chief replicas take the chief's variables, slots, beta powers and global_step."""
        self.gather_state()
        for g in self.groups.values():
            for buf in (g.var, g.m, g.v):
                if buf is not None:        # 'momentum' keeps no v
                    dist.broadcast(buf, src)
        powers = self._broadcast_step(dist, src, [float(x) for g in self.groups.values()
                                                  for x in (g.beta1_power, g.beta2_power)])
        for i, g in enumerate(self.groups.values()):
            g.beta1_power, g.beta2_power = np.float32(powers[2 * i]), np.float32(powers[2 * i + 1])
        if self.wcopy:
            self.refresh_weight_copies()
        self._refresh_prepared()

    def _kb(self, name):
        return self._v(name + '/kernel'), self._v(name + '/bias')

    FEW_CHANNEL = ('coarse/conv/conv2d_0', 'fine/first/conv2d')

    def _fwd_operands(self, name):
        d, w = self._desc(name, 'fwd'), self._w(name)
        if name in self.FEW_CHANNEL:
            d, w = self._prepared((name, d.storage, d.hints, d.precision), d, w)
        return d, w

    def _conv(self, name, x, y):
        d, w = self._fwd_operands(name)
        ops.conv2d_fwd(d, x, w, self._v(name + '/bias'), y, 'relu' if self.conv[name].relu else None)

    @contextlib.contextmanager
    def _beside(self):
        """Enqueue the body on the side stream, ordered after everything enqueued on the current stream so far."""
        if self.side is None:
            yield
            return
        self.side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.side):
            yield

    def _join(self):
        if self.side is not None:
            torch.cuda.current_stream().wait_stream(self.side)

    # ---- forward: src/models.py:277-290 ----
    def prepool_equivalent(self, which):
        """'c0' | 'c1' | 'f1' as far as a backward pass can tell: the tensor itself when the last forward wrote it,
        otherwise zeros with each pool window's maximum at its recorded position (same MaxPoolGrad routing, same
        ReluGrad mask).  For tests and debugging."""
        src = {'c0': (self.c0, self.p0, self.a0, 1), 'c1': (self.c1, self.p1, self.a1, 1),
               'f1': (self.f1, self.cat, self.af1, 2)}[which]
        full, pooled, arg, phase = src
        if self.pooled_fwd != phase and not self.bf16s:
            return full
        if full is None:          # 'bf16s': the tensor does not exist at all
            full = torch.empty((pooled.shape[0],) + {'c0': (55, 74, 96), 'c1': (27, 37, 256), 'f1': (110, 148, 63)}[which],
                               device=self.device)
        pooled = pooled.float()
        c = arg.shape[-1]
        out = torch.zeros_like(full)
        ph, pw = arg.shape[1], arg.shape[2]
        win = out[:, :2 * ph, :2 * pw, :].reshape(full.shape[0], ph, 2, pw, 2, c)
        a = arg.long()
        for pos in range(4):
            win[:, :, pos >> 1, :, pos & 1, :] = torch.where(a == pos, pooled[..., :c], torch.zeros_like(pooled[..., :c]))
        return out

    def _conv_pool(self, name, x, y_pooled, argmax=None):
        d, w = self._fwd_operands(name)
        ops.conv2d_pool_fwd(d, x, w, self._v(name + '/bias'), y_pooled, 'relu', argmax)

    def _fine_first_image_form(self, argmax=None):
        """'bf16s': fine/first on the bf16 pipe from the 4-channel bf16 image, conv + ReLU + pool in one launch."""
        d, w = self._prepared(('fine/first/image', 0, 0, 0), self.d4, self.w4)
        ops.conv2d_pool_fwd(d, self.x4, w, self._v('fine/first/conv2d/bias'), self.cat, 'relu', argmax)

    def forward(self, images, depths, keep_mask, join=True, phase=None, warp=None):
        """join=False leaves the fine network's forward in flight on the side stream (step() joins later).
        phase (1 coarse / 2 fine / 3 none trained) runs every conv that feeds a max pool fused with it: the pre-pool
        activations c0, c1, f1 are then NOT written.  The network being trained also records the position of each
        maximum (a0, a1 / af1): MaxPoolGrad routes dy to that position and the fused ReluGrad only asks whether the
        maximum is positive, so the backward needs nothing else of c0 / c1 / f1.  phase None keeps every activation.
        depths None (predict()): the input images are already in self.x, no target is resized and no loss computed.
        warp (NON-REFERENCE, train-time augmentation): a device table [B, 12] of ops.warp_bilinear_pair, which then takes
        the place of the resize launch; images and depths are stored at the same size."""
        if depths is None:
            pass
        elif self.valid_range is not None:
            lo, hi = self.valid_range
            if warp is not None:
                ops.warp_bilinear_pair_valid(images, self.x, depths, self.t, warp, lo, hi)
            elif images.shape[:3] == depths.shape[:3]:
                ops.resize_bilinear_tf1_pair_valid(images, self.x, depths, self.t, lo, hi)
            else:
                ops.resize_bilinear_tf1(images, self.x)
                ops.resize_bilinear_tf1_valid(depths, self.t, lo, hi, scratch=self.t_one)
        elif warp is not None:
            ops.warp_bilinear_pair(images, self.x, depths, self.t, warp)
        elif images.shape[:3] == depths.shape[:3]:
            ops.resize_bilinear_tf1_pair(images, self.x, depths, self.t)
        else:
            ops.resize_bilinear_tf1(images, self.x)
            ops.resize_bilinear_tf1(depths, self.t)
        B = self.B
        self.dropout_on = keep_mask is not None            # None: the plugin was called with train=False
        # fine phase: the main queue has nothing left to run beside fine/second (the coarse backward does not exist there and
        # the fine backward waits for this forward), so the launch takes the whole CU instead of leaving room (A3D_HINT_SHARE_CU)
        self._alone = ('fine/second/conv2d',) if phase == 2 else ()
        if self.bf16s:
            # the 4-channel bf16 image of conv2d_0's and fine/first's forwards, on the main stream: the side stream's chain
            # (fine/first .. loss) is the longer one at the join, the main stream idles there
            ops.pad_channels_bf16(self.x, self.x4)
        fused = self.fuse_pool and phase in (1, 2, 3)
        self.pooled_fwd = phase if fused else None
        lean_fine = fused
        if fused:
            train = phase == 1
            self._conv_pool('coarse/conv/conv2d_0', self.x, self.p0, self.a0 if train else None)
            self._conv_pool('coarse/conv/conv2d_1', self.p0, self.p1, self.a1 if train else None)
        elif self.bf16s:
            d, w = self._prepared(('conv2d_0/image', 0, 0, 0), self.d0_4, self.w0_4)
            ops.conv2d_pool_fwd(d, self.x4, w, self._v('coarse/conv/conv2d_0/bias'), self.p0, 'relu', self.a0)
            # conv + ReLU + pool in the LDS-DMA kernel's epilogue: c1 (33 MB at B = 64) is never written
            self._conv_pool('coarse/conv/conv2d_1', self.p0, self.p1, self.a1)
        else:
            self._conv('coarse/conv/conv2d_0', self.x, self.c0)
            ops.maxpool2x2_fwd(self.c0, self.p0)
            self._conv('coarse/conv/conv2d_1', self.p0, self.c1)
            ops.maxpool2x2_fwd(self.c1, self.p1)
        def fine_first():
            with self._beside():    # beside the two weight-streaming dense layers
                if lean_fine:
                    self._conv_pool('fine/first/conv2d', self.x, self.cat, self.af1 if phase == 2 else None)   # cat[..., :63]
                elif self.bf16s:    # conv + ReLU + pool in one launch: f1 is never written; where the layer trains (not in
                    # phases 1 and 3) it also records the window positions
                    self._fine_first_image_form(None if phase in (1, 3) else self.af1)
                else:
                    self._conv('fine/first/conv2d', self.x, self.f1)
        # where the side stream starts: ahead of conv2d_4's forward.  The fine forward is the longer chain of the stretch
        # (bf16 storage: fine/first runs 0.27 ms beside the dense layers; started after conv2d_4 it left the main queue
        # waiting 41 us at the join: 1.43 -> 1.39 ms; fp32: 26 us at the join, 2.93 -> 2.91 ms).  One layer earlier still is
        # slower again (1.41 / 2.94 ms), two layers 1.44: MFMA-bound grids beside each other only trade CU slots.
        self._conv('coarse/conv/conv2d_2', self.p1, self.c2)
        self._conv('coarse/conv/conv2d_3', self.c2, self.c3)
        fine_first()
        self._c4_32_fresh = False
        if self.bf16s and self.dense_bf16_x and phase == 1:
            # c4 also as float32 (dense_0's filter gradient reads it in that type) from the same reduction
            n4 = 'coarse/conv/conv2d_4'
            ops.conv2d_fwd(self._desc(n4, 'fwd'), self.c3, self._w(n4), self._v(n4 + '/bias'), self.c4, 'relu',
                           out2=ops.second_output(self.c4_32.view(-1, 256)))
            self._c4_32_fresh = True
        else:
            self._conv('coarse/conv/conv2d_4', self.c3, self.c4)
        if not self._sharded_in_flight():
            self.settle()           # the previous step's dense-layer update is due now, not earlier
        w, b = self._kb('coarse/dense/dense_0')
        if self.bf16s and self.dense_bf16_x:   # dense_0 streams its 100 MB bf16 weight copy against c4 as it stands (bf16): LDS-DMA kernel
            # (its bf16 copy for dense_1 leaves through the same reduction: a3d_second_output, round 5)
            ops.dense_fwd_ex(self.c4.view(B, -1), self.wcopy['coarse/dense/dense_0'], b, self.drop, 'relu',
                             drop_keep=keep_mask, precision='bf16', storage=ops.STORE_W | ops.STORE_X,
                             out2=ops.second_output(self.drop16))
        elif self.bf16s:            # more than 64 rows: the LDS-DMA kernel's weight-stream tiles do not apply; fp32 x, bf16 weight copy
            ops.cast_bf16(self.c4, self.c4_32)
            ops.dense_fwd_ex(self.c4_32.view(B, -1), self.wcopy['coarse/dense/dense_0'], b, self.drop, 'relu',
                             drop_keep=keep_mask, precision='bf16', storage=ops.STORE_W)
        else:
            ops.dense_fwd(self.c4.view(B, -1), w, b, self.drop, 'relu', drop_keep=keep_mask)     # relu + dropout fused
        w, b = self._kb('coarse/dense/dense_1')
        cat_done = self.bf16s and self.dense_bf16_x
        if cat_done:
            # the padded GEMM (4072 columns) writes the 4070-column depth map AND channel 63 of the concat buffer from its
            # reduction: no cast_rows, no copy_channel launch
            ops.dense_fwd_ex(self.drop16, self.w1pad, self.b1pad, self.coarse.view(B, -1), None, precision='bf16',
                             storage=ops.STORE_W | ops.STORE_X, n=self.w1pad.shape[1],
                             out2=ops.second_output(self.cat, cols=OUT_H * OUT_W, step=64, offset=63, ld=OUT_H * OUT_W))
        else:
            ops.dense_fwd(self.drop, w, b, self.coarse.view(B, -1))
        with self._beside():
            if cat_done:
                pass
            elif lean_fine or self.bf16s:
                ops.copy_channel(self.coarse, 0, self.cat, 63)                                # tf.concat([pool, coarse])
            else:
                ops.maxpool2x2_fwd(self.f1, self.cat, extra=self.coarse)                      # pool + concat fused
            self._conv('fine/second/conv2d', self.cat, self.f2)
            self._conv('fine/third', self.f2, self.fine)
            if depths is not None:
                self._loss_fwd(self.fine, self.loss_out_f, self.ws_f)
        if depths is not None:
            self._loss_fwd(self.coarse, self.loss_out_c, self.ws_c)
        if join:
            self._join()

    def predict(self, images, n=None):
        """The network's depth maps for a batch of images, without targets: (coarse, fine), each [B, 55, 74] float32
        (views of this replica's buffers, valid until its next forward).  images [m, H, W, 3] float32, or the uint8 pixel
        values of converter-written records, m <= B; only rows [0, n) (default m) are read, rows n .. B of the network
        input are zero, so a short last batch runs at the replica's B and its rows [0, n) are those of a full batch.
        The phase-3 forward (conv + pool fused, no argmax recorded) with dropout off, tf.layers.dropout(training=False)
        (src/models.py:230).  Weights, gradients, Adam slots and global_step are left as they are; the side stream is
        joined before returning."""
        B = self.B
        n = images.shape[0] if n is None else int(n)
        check_rows('predict', n, B, f'a batch of {images.shape[0]} images', images.shape[0])
        ops.resize_bilinear_tf1(images[:n], self.x[:n])
        if n < B:
            self.x[n:].zero_()
        self.forward(images, None, None, join=True, phase=3)
        return self.coarse.view(B, OUT_H, OUT_W), self.fine.view(B, OUT_H, OUT_W)

    def _loss_fwd(self, out, loss, ws):
        """One launch: the loss of `out` against self.t into `loss`, the buffer that launch writes (loss_out_c / loss_out_f)."""
        self._loss.fwd(out, self.t, loss, ws)

    def _loss_bwd(self, out, ws, dout, dout16=None):
        self._loss.bwd(out, self.t, ws, dout, dout16)

    def _sharded_in_flight(self):
        """The deferred dense bucket is a reduce-scatter feeding only the m slot: nothing in the forward needs it, it is due
        when the next backward is about to overwrite the gradient buffer it reads (backward_coarse settles first)."""
        d = self._deferred
        return d is not None and bool(d[0]) and isinstance(d[0][0], tuple)

    def _fused_dense_adam(self):
        return not self.keep_dense_grads and self.groups['CoarseDense'].frozen()

    def _fused_dense_momentum(self):
        return not self.keep_dense_grads and self.optimizer == 'momentum'

    def _bwd_data(self, name, dz, dx, relu_mask=None):
        d, w = self._desc(name, 'bwd_d'), self._w(name, 'bwd_d')
        if name in self.d_wino:
            d, w = self._prepared((name, 'bwd_d', 'fp32w'), self.d_wino[name], w, 'bwd_d')
        if name in self.wino1d_bwd_d:
            d, w = self._prepared((name, 'bwd_d', 'wino1d'), d, w, 'bwd_d_wino1d')
            ops.conv2d_bwd_data_wino1d(d, dz, w, dx, relu_mask=relu_mask)
            return
        ops.conv2d_bwd_data(d, dz, w, dx, relu_mask=relu_mask)

    def _wino_chain(self, name):
        """Both Winograd routes are on for the layer: its two gradients run as one chain (ops.conv2d_bwd_wino)."""
        return self.WINO_BWD_CHAIN and name in self.d_wino and name in self.wino_grad

    def _bwd_wino(self, name, x, dz, dx, relu_mask=None, pool=None):
        d, w = self._prepared((name, 'bwd_d', 'fp32w'), self.d_wino[name], self._w(name, 'bwd_d'), 'bwd_d')
        ops.conv2d_bwd_wino(d, x, dz, w, self._g(name + '/kernel'), self._g(name + '/bias'), dx, relu_mask=relu_mask, pool=pool)

    def _bwd_filter(self, name, x, dz):
        if name in self.d:
            call = ops.conv2d_bwd_filter_wino if name in self.wino_grad else ops.conv2d_bwd_filter
            if name in self.wino1d_bwd_f:
                call = ops.conv2d_bwd_filter_wino1d
            call(self._desc(name, 'bwd_f'), x, dz, self._g(name + '/kernel'), self._g(name + '/bias'))
        elif self._fused_dense_adam():
            g = self.groups[self.group_of[name + '/kernel']]
            kw = [g.view(buf, name + '/kernel') for buf in (g.var, g.m, g.v)]
            kb = [g.view(buf, name + '/bias') for buf in (g.var, g.m, g.v)]
            ops.dense_bwd_filter_adam_tf1(x, dz, *kw, *kb, g.lr, g.beta1, g.beta2, float(g.beta1_power),
                                          float(g.beta2_power), 1.0, precision='bf16' if self.bf16s else 'fp32')
        elif self._fused_dense_momentum():
            g = self.groups[self.group_of[name + '/kernel']]
            slots = [g.view(buf, name + which) for which in ('/kernel', '/bias') for buf in (g.var, g.m)]
            ops.dense_bwd_filter_momentum(x, dz, *slots, g.lr, g.momentum, 1.0)
        else:
            ops.dense_bwd_filter(x, dz, self._g(name + '/kernel'), self._g(name + '/bias'))

    # ---- backward of loss_coarse wrt coarse/* : src/models.py:318-324 ----
    def backward_coarse(self, after_dense=None, after_conv2=None, after_dense1=None):
        B = self.B
        bf16_x = self.bf16s and self.dense_bf16_x
        self._loss_bwd(self.coarse, self.ws_c, self.dz1.view(B, OUT_H, OUT_W, 1),
                       dout16=self.dz1_16 if bf16_x else None)   # (dz1 a second time as bf16 rows of 4072: dense_1's bwd-data)
        self.settle()              # a reduce-scatter of the previous step may still be reading the dense gradient buffer
        n = 'coarse/dense/dense_1'
        # the fused momentum launch moves the layer's kernel: it runs after the bwd-data that must still read the old one
        # (the reference's frozen Adam never moves it, and every other path applies after the backward)
        late = self._fused_dense_momentum()
        if not late:
            self._bwd_filter(n, self.drop, self.dz1)
        if after_dense1 is not None:
            after_dense1()         # dense_1's gradient (67 MB) is complete: first piece of the dense bucket
        # dropout-grad (x2 on kept units) and dense_0's ReluGrad in one mask: drop > 0  <=>  kept and relu active
        # (train=False, src/models.py:230: tf.layers.dropout is the identity; only the ReluGrad remains)
        if bf16_x:
            ops.dense_bwd_data_ex(self.dz1_16, self.w1pad, self.dz0, mask=self.drop, scale=2.0 if self.dropout_on else 1.0,
                                  precision='bf16', storage=ops.STORE_W | ops.STORE_Y,
                                  out2=ops.second_output(self.dz0_16))     # dz0 as bf16 too: dense_0's bwd-data
        else:
            ops.dense_bwd_data(self.dz1, self._v(n + '/kernel'), self.dz0, mask=self.drop, scale=2.0 if self.dropout_on else 1.0)
        if late:
            self._bwd_filter(n, self.drop, self.dz1)
        n = 'coarse/dense/dense_0'
        if bf16_x and not self._c4_32_fresh:    # the filter gradient takes c4 on the dense layers' fp32 side
            ops.cast_bf16(self.c4, self.c4_32)      # (B > 64: the forward already made this copy; phase 1: conv2d_4's reduction did)
        flat = (self.c4_32 if self.bf16s else self.c4).view(B, -1)
        if not late:
            self._bwd_filter(n, flat, self.dz0)
        if bf16_x:      # dc4 leaves as bf16, masked by the bf16 c4: no fp32 detour
            ops.dense_bwd_data_ex(self.dz0_16, self.wcopy[n], self.dc4.view(B, -1), mask=self.c4.view(B, -1), scale=1.0,
                                  precision='bf16', storage=ops.STORE_W | ops.STORE_X | ops.STORE_Y)
        elif self.bf16s:            # B > 64: fp32 dz0 and mask against the bf16 weight copy, dc4 through an fp32 buffer
            ops.dense_bwd_data_ex(self.dz0, self.wcopy[n], self.dc4_32.view(B, -1), mask=flat, scale=1.0, precision='bf16',
                                  storage=ops.STORE_W)
            ops.cast_bf16(self.dc4_32, self.dc4)
        else:
            ops.dense_bwd_data(self.dz0, self._v(n + '/kernel'), self.dc4.view(B, -1), mask=flat, scale=1.0)
        if late:
            self._bwd_filter(n, flat, self.dz0)
        if after_dense is not None:
            after_dense()          # dense gradients are complete: their all-reduce can overlap the conv backward
        n = 'coarse/conv/conv2d_4'
        self._bwd_filter(n, self.c3, self.dc4)
        self._bwd_data(n, self.dc4, self.dc3, relu_mask=self.c3)
        self._join()               # the fine forward has had the dense / conv2d_4 stretch; the big GEMMs below run alone
        # (round 4: the join costs the main queue ~25 us — the side stream's loss kernel ends 14 us after conv2d_4's backward,
        # plus the cross-queue signal.  Joining later — after conv2d_3's filter gradient, after its bwd-data, at the end of the
        # backward — was measured at 2.97 ms against 2.92: a stream-K grid sized for all CU slots starts lopsided when the
        # side stream's blocks still hold some.  bf16 storage: 1.504 against 1.506, noise.)
        # (measured, round 3: the filter-gradient GEMMs on the side stream beside the bwd-data chain — to fill its tails and
        # launch gaps — make the step 2 % SLOWER, 3.20 vs 3.14 ms: two MFMA-bound grids only take CU slots from each other)
        dw = self._bwd_filter
        pooled = self.pooled_fwd == 1 or self.bf16s         # the forward recorded a0 / a1 instead of writing c0 / c1
        n = 'coarse/conv/conv2d_3'
        if self._wino_chain(n):
            self._bwd_wino(n, self.c2, self.dc3, self.dc2, relu_mask=self.c2)
        else:
            dw(n, self.c2, self.dc3)
            self._bwd_data(n, self.dc3, self.dc2, relu_mask=self.c2)
        n = 'coarse/conv/conv2d_2'
        if self._wino_chain(n):
            # one chain: dw, db and — where the fused forward recorded a1 — dc1 itself, the pool's gradient scattered by the
            # output transform (dp1 is never written).  after_conv2 fires one product launch later than on the separate calls
            self._bwd_wino(n, self.p1, self.dc2, self.dc1 if pooled else self.dp1, pool=(self.a1, self.p1) if pooled else None)
            if after_conv2 is not None:
                after_conv2()
            if not pooled:
                ops.maxpool2x2_bwd(self.c1, self.dp1, self.dc1, relu_mask=True)
        else:
            dw(n, self.p1, self.dc2)
            if after_conv2 is not None:
                after_conv2()          # gradients of conv2d_2..4 (the tail of the CoarseConv buffer) are complete
            self._bwd_data(n, self.dc2, self.dp1)
            if pooled:
                ops.maxpool2x2_bwd_idx(self.a1, self.p1, self.dp1, self.dc1, relu_mask=True)
            else:
                ops.maxpool2x2_bwd(self.c1, self.dp1, self.dc1, relu_mask=True)
        n = 'coarse/conv/conv2d_1'
        dw(n, self.p0, self.dc1)
        self._bwd_data(n, self.dc1, self.dp0)
        n = 'coarse/conv/conv2d_0'
        if pooled and n in self.d_few:
            ops.conv2d_bwd_filter_pooled(self.d_few[n], self.x, self.dp0, self.p0, self.a0, self._g(n + '/kernel'),
                                         self._g(n + '/bias'))
            return
        if self.dc0 is None:
            self.dc0 = torch.empty((self.B, 55, 74, 96), device=self.device, dtype=self.dp0.dtype)
        if pooled:
            ops.maxpool2x2_bwd_idx(self.a0, self.p0, self.dp0, self.dc0, relu_mask=True)
        else:
            ops.maxpool2x2_bwd(self.c0, self.dp0, self.dc0, relu_mask=True)
        dw(n, self.x, self.dc0)

    # ---- backward of loss_fine wrt fine/* : src/models.py:333-338 ----
    def backward_fine(self):
        self._join()                                                          # the fine forward ran on the side stream
        self._loss_bwd(self.fine, self.ws_f, self.dfine)
        n = 'fine/third'
        if ops.conv2d_bwd_both_supported(self.d[n]):
            # filter, bias and input gradient (+ fine/second's ReluGrad) in one pass over f2
            ops.conv2d_bwd_both(self.d[n], self.f2, self.dfine, self._v(n + '/kernel'), self._g(n + '/kernel'),
                                self._g(n + '/bias'), self.df2, relu_mask=True)
        else:
            assert not self.bf16s, 'bf16 storage: df2 is a bf16 tensor only the fused backward writes'
            self._bwd_filter(n, self.f2, self.dfine)
            self._bwd_data(n, self.dfine, self.df2, relu_mask=self.f2)
        n = 'fine/second/conv2d'
        self._bwd_filter(n, self.cat, self.df2)
        self._bwd_data(n, self.df2, self.dcat)
        n = 'fine/first/conv2d'
        if (self.pooled_fwd == 2 or self.bf16s) and n in self.d_few:          # reads channels 0..62 of dcat / cat
            ops.conv2d_bwd_filter_pooled(self.d_few[n], self.x, self.dcat, self.cat, self.af1, self._g(n + '/kernel'),
                                         self._g(n + '/bias'))
            return
        if self.df1 is None:
            self.df1 = torch.empty((self.B, 110, 148, 63), device=self.device)
        if self.pooled_fwd == 2 or self.bf16s:                                 # both read channels 0..62 of dcat
            ops.maxpool2x2_bwd_idx(self.af1, self.cat, self.dcat, self.df1, relu_mask=True)
        else:
            ops.maxpool2x2_bwd(self.f1, self.dcat, self.df1, relu_mask=True)
        self._bwd_filter(n, self.x, self.df1)

    # ---- one session.run(train_op) ----
    def step(self, images, depths, keep_mask, warp=None):
        """images [B,H,W,3], depths [B,H',W',1] float32, keep_mask [B,4096] bool/uint8, all on this device.
        Both forwards and both losses run in every phase; gradients + Adam only for the active phase;
        global_step += 1 always (src/models.py:329,343,356).  warp: see forward()."""
        if keep_mask is not None and keep_mask.dtype != torch.uint8:
            keep_mask = keep_mask.to(torch.uint8)
        phase = phase_of(self.global_step, self.B)
        self.forward(images, depths, keep_mask, join=False, phase=phase, warp=warp)
        red = self.reducer
        scale = 1.0 / red.world_size if red is not None else 1.0
        if phase == 1:
            gc, gd = self.groups['CoarseConv'], self.groups['CoarseDense']
            if red is None:
                fused = self._fused_dense_adam() or self._fused_dense_momentum()      # decided before the backward: it is what the dense layers ran
                self.backward_coarse()
                gc.apply(scale)
                if fused:
                    gd.advance()                       # the update of coarse/dense/* already happened inside the backward
                else:
                    gd.apply(scale)
                self._weights_moved(gc, gd)
            else:
                # dense bucket (268 MB): reduced while the conv backward runs AND, being due only before the next
                # step's dense_0, while that step's conv forward runs (settle()); conv bucket (15 MB): waited for here
                # conv bucket in two pieces: conv2d_2..4 (12.4 of 15 MB, the tail of the flat buffer) goes out as
                # soon as conv2d_2's filter gradient exists and rides under the conv2d_1 / conv2d_0 backward; only
                # the 2.6 MB head is reduced on the critical path
                handle, tail = [], []
                cut = gc.offsets['coarse/conv/conv2d_2/kernel'][0]
                if gd.frozen() and self.dense_exchange == 'reduce_scatter':
                    # the reference's optimizer: reduce-scatter, each rank updates m on its own slices only (dp.py)
                    early, late = self._dense_buckets()
                    if self._poison is None:
                        self._poison = torch.zeros(1, dtype=torch.int32, device=self.device)

                    def scatter(pieces):
                        for a, b in pieces:
                            work, _ = red.reduce_scatter(gd.grad[a:b])
                            handle.append((work,) + self._my_slice(a, b))
                    after_dense1, after_dense = (lambda: scatter(early)), (lambda: scatter(late))
                else:
                    # dense bucket in backward production order: dense_1 (67 MB) leaves as soon as its filter
                    # gradient exists, dense_0 (201 MB) in three pieces after its own — four collectives of 50-67 MB
                    # pipeline over the xGMI links where one 268 MB ring would serialise behind its own reduce-scatter
                    d1 = gd.offsets['coarse/dense/dense_1/kernel'][0]
                    third = -(-(d1 // 3) // ParamGroup.ALIGN) * ParamGroup.ALIGN
                    pieces0 = [(0, third), (third, 2 * third), (2 * third, d1)]
                    after_dense1 = lambda: handle.append(red.start(gd.grad[d1:]))
                    after_dense = lambda: handle.extend(red.start(gd.grad[a:b]) for a, b in pieces0)
                self.backward_coarse(after_dense1=after_dense1, after_dense=after_dense,
                                     after_conv2=lambda: tail.append(red.start(gc.grad[cut:], urgent=True)))
                head = red.start(gc.grad[:cut], urgent=True)       # (urgent: not queued behind the dense reduce-scatter, dp.py)
                red.wait(tail[0])
                red.wait(head)
                gc.apply(scale)
                self._weights_moved(gc)
                self._deferred = (handle, gd, scale)
        elif phase == 2:
            ga, gb = self.groups['FineA'], self.groups['FineB']
            self.backward_fine()
            if red is not None:
                red.start(ga.grad)
                red.start(gb.grad)
                red.finish()
            ga.apply(scale)
            gb.apply(scale)
            self._weights_moved(ga, gb)
        self._join()
        self.global_step += 1
        return {'coarse_loss': self.loss_coarse, 'fine_loss': self.loss_fine, 'phase': phase}


# =====================================================================================================
# DCNF unary stack ("DCNF-lite", Liu et al. 2015) — src/models.py:14-18,50-89,179-183
# =====================================================================================================
DCNF_IMG_H, DCNF_IMG_W = 240, 320      # src/models.py:180
DCNF_PATCH, DCNF_SP = 100, 40          # src/models.py:15-16
DCNF_PREFIX = 'unary/unary_layers/'
DCNF_CONVS = [('conv2d', 3, 64, 11), ('conv2d_1', 64, 256, 5), ('conv2d_2', 256, 256, 3),
              ('conv2d_3', 256, 256, 3), ('conv2d_4', 256, 256, 3)]        # all VALID, stride 1, ReLU (:64-72)
DCNF_POOL_AFTER = ('conv2d', 'conv2d_1', 'conv2d_4')                       # :65,68,73
DCNF_DENSES = [('dense', 12544, 128, 'relu'), ('dense_1', 128, 16, 'sigmoid'), ('dense_2', 16, 1, None)]  # :80-82


class DCNFUnary:
    """The shared-weight unary conv stack over all patches of a batch at once (the reference maps it over the
    batch with tf.map_fn, src/models.py:89): images [B,H,W,3] -> z [B,48,1].  backward() takes a synthetic
    upstream gradient dz (DCNFReplica feeds it the CRF loss gradient)."""

    def __init__(self, batchsize, device='cuda', params=None, seed=3000, precision='fp32'):
        self.B = batchsize
        self.device = dev = torch.device(device)
        self.rows, _ = ops.same_pad(DCNF_IMG_H, DCNF_PATCH, DCNF_SP)
        self.cols, _ = ops.same_pad(DCNF_IMG_W, DCNF_PATCH, DCNF_SP)
        self.P = P = batchsize * self.rows * self.cols
        shapes = collections.OrderedDict()
        for n, ci, co, k in DCNF_CONVS:
            shapes[DCNF_PREFIX + n + '/kernel'] = (k, k, ci, co)
            shapes[DCNF_PREFIX + n + '/bias'] = (co,)
        for n, i, o, _ in DCNF_DENSES:
            shapes[DCNF_PREFIX + n + '/kernel'] = (i, o)
            shapes[DCNF_PREFIX + n + '/bias'] = (o,)
        self.shapes = shapes
        self.group = ParamGroup('unary', 0.1, shapes, dev, slots=False)    # GradientDescentOptimizer(0.1), src/models.py:198
        if params is None:
            rng = np.random.default_rng(seed)
            params = {n: (glorot_uniform(rng, s) if n.endswith('/kernel') else np.zeros(s, np.float32))
                      for n, s in shapes.items()}
        for n, s in shapes.items():
            self.group.view(self.group.var, n).copy_(torch.from_numpy(np.ascontiguousarray(params[n], np.float32)))

        def buf(*shape):
            return torch.empty(shape, device=dev)
        self.resized = buf(batchsize, DCNF_IMG_H, DCNF_IMG_W, 3)
        self.act = collections.OrderedDict()
        self.dact = {}
        self.desc = {}
        # conv + ReLU + max pool in one kernel (fp32): the pre-pool activations (1.6 + 1.3 GB at batch 16) are never
        # written, one argmax byte per pool window serves the backward (see MSDNReplica.forward)
        self.fuse_pool = precision == 'fp32'
        self.argmax, self.conv_hw = {}, {}
        self.few_pooled = False
        self.act['x'] = buf(P, DCNF_PATCH, DCNF_PATCH, 3)
        h = DCNF_PATCH
        for n, ci, co, k in DCNF_CONVS:
            self.desc[n] = ops.conv_desc(P, h, h, ci, co, k, k, 1, 'VALID', precision=precision)
            h = h - k + 1
            self.conv_hw[n] = h
            if not (self.fuse_pool and n in DCNF_POOL_AFTER):
                self.act[n] = buf(P, h, h, co)
            if n in DCNF_POOL_AFTER:
                h //= 2
                self.act[n + '/pool'] = buf(P, h, h, co)
                if self.fuse_pool:
                    self.argmax[n] = torch.empty((P, h, h, co), dtype=torch.uint8, device=dev)
        for n, i, o, _ in DCNF_DENSES:
            self.act[n] = buf(P, o)
        self.z = self.act['dense_2']
        self.few_pooled = (self.fuse_pool and dev.type == 'cuda'
                           and ops.conv2d_bwd_filter_pooled_supported(self.desc['conv2d']))

    def var(self, name):
        return self.group.view(self.group.var, DCNF_PREFIX + name)

    def grad(self, name):
        return self.group.view(self.group.grad, DCNF_PREFIX + name)

    def forward(self, images, record_argmax=True):
        ops.resize_bilinear_tf1(images, self.resized)                           # src/models.py:180
        return self.forward_resized(record_argmax)

    def forward_resized(self, record_argmax=True):
        """The stack over self.resized as it stands.  record_argmax=False (DCNFReplica.predict): the fused conv + pool
        does not write the pool positions, which only a backward reads."""
        ops.extract_patches(self.resized, DCNF_PATCH, DCNF_SP, self.act['x'])   # :50-59
        t = self._forward_convs(self.act['x'], record_argmax)
        self._forward_denses(t.view(self.P, -1))
        return self.z.view(self.B, self.rows * self.cols, 1)

    def _forward_convs(self, t, record_argmax):
        for n, _, _, _ in DCNF_CONVS:
            if self.fuse_pool and n in DCNF_POOL_AFTER:
                t = ops.conv2d_pool_fwd(self.desc[n], t, self.var(n + '/kernel'), self.var(n + '/bias'),
                                        self.act[n + '/pool'], 'relu', self.argmax[n] if record_argmax else None)
                continue
            ops.conv2d_fwd(self.desc[n], t, self.var(n + '/kernel'), self.var(n + '/bias'), self.act[n], 'relu')
            t = self.act[n]
            if n in DCNF_POOL_AFTER:
                ops.maxpool2x2_fwd(t, self.act[n + '/pool'])
                t = self.act[n + '/pool']
        return t

    def _forward_denses(self, t):
        for n, _, _, act in DCNF_DENSES:
            ops.dense_fwd(t, self.var(n + '/kernel'), self.var(n + '/bias'), self.act[n], act)
            t = self.act[n]

    def activations(self):
        """name -> numpy array of every activation; a pre-pool activation that the fused conv + pool never wrote comes
        back as zeros with each window's maximum at its recorded position (all a backward pass can see of it)."""
        out = {k: v.cpu().numpy() for k, v in self.act.items()}
        for n, arg in self.argmax.items():
            pooled = self.act[n + '/pool']
            (hh, ww), c = self._conv_hw(n), pooled.shape[-1]
            N, ph, pw = pooled.shape[:3]
            full = torch.zeros((N, hh, ww, c), device=self.device)
            win = full[:, :2 * ph, :2 * pw, :].reshape(N, ph, 2, pw, 2, c)
            a = arg.long()
            for pos in range(4):
                win[:, :, pos >> 1, :, pos & 1, :] = torch.where(a == pos, pooled, torch.zeros_like(pooled))
            out[n] = full.cpu().numpy()
        return out

    def _conv_hw(self, n):
        """(height, width) of conv n's output."""
        hw = self.conv_hw[n]
        return hw if isinstance(hw, tuple) else (hw, hw)

    def _dbuf(self, key, like):
        if key not in self.dact:
            self.dact[key] = torch.empty_like(like)
        return self.dact[key]

    def backward(self, dz):
        """Gradients of sum(z * dz) wrt every unary variable, into the flat gradient buffer."""
        P = self.P
        a = self.act
        flat = a['conv2d_4/pool'].view(P, -1)
        d0 = self._backward_denses(flat, dz)
        dflat = self._dbuf('flat', a['conv2d_4/pool'])
        ops.dense_bwd_data(d0, self.var('dense/kernel'), dflat.view(P, -1))
        self._backward_convs(dflat)

    def _backward_denses(self, flat, dz):
        """The three dense layers' gradients from dz, flat [P, in] being the first one's input; returns the gradient of
        the first layer's pre-activation, which the caller takes on to flat's own gradient."""
        P = self.P
        a = self.act
        d2 = dz.reshape(P, 1).contiguous()
        # dense_2 (linear)
        ops.dense_bwd_filter(a['dense_1'], d2, self.grad('dense_2/kernel'), self.grad('dense_2/bias'))
        d1 = self._dbuf('dense_1', a['dense_1'])
        ops.dense_bwd_data(d2, self.var('dense_2/kernel'), d1, mask=a['dense_1'], mask_act='sigmoid')  # y(1-y) fused
        ops.dense_bwd_filter(a['dense'], d1, self.grad('dense_1/kernel'), self.grad('dense_1/bias'))
        d0 = self._dbuf('dense', a['dense'])
        ops.dense_bwd_data(d1, self.var('dense_1/kernel'), d0, mask=a['dense'], scale=1.0)     # ReluGrad fused
        ops.dense_bwd_filter(flat, d0, self.grad('dense/kernel'), self.grad('dense/bias'))
        return d0

    def _backward_convs(self, d):
        """The five convs' gradients from d, the gradient of conv2d_4/pool."""
        a = self.act
        N = a['x'].shape[0]
        inputs = {'conv2d': 'x', 'conv2d_1': 'conv2d/pool', 'conv2d_2': 'conv2d_1/pool', 'conv2d_3': 'conv2d_2',
                  'conv2d_4': 'conv2d_3'}
        for n, _, _, _ in reversed(DCNF_CONVS):
            if n == 'conv2d' and self.fuse_pool and self.few_pooled:
                # the first conv's filter gradient straight from the pooled map's gradient: its 768 x 90 x 90 x 64 pre-pool
                # gradient (1.6 GB at batch 16) is never written
                pool = a[n + '/pool']
                ops.conv2d_bwd_filter_pooled(self.desc[n], a['x'], d.view(pool.shape), pool, self.argmax[n],
                                             self.grad(n + '/kernel'), self.grad(n + '/bias'))
                continue
            if n in DCNF_POOL_AFTER and self.fuse_pool:
                (hh, ww), co = self._conv_hw(n), a[n + '/pool'].shape[-1]
                if n not in self.dact:
                    self.dact[n] = torch.empty((N, hh, ww, co), device=self.device)
                dzc = self.dact[n]
                ops.maxpool2x2_bwd_idx(self.argmax[n], a[n + '/pool'], d.view(a[n + '/pool'].shape), dzc, relu_mask=True)
            elif n in DCNF_POOL_AFTER:
                dzc = self._dbuf(n, a[n])
                ops.maxpool2x2_bwd(a[n], d, dzc, relu_mask=True)
            else:
                dzc = d      # the producer (bwd-data of the next conv) already applied this layer's ReluGrad
            x = a[inputs[n]]
            ops.conv2d_bwd_filter(self.desc[n], x, dzc, self.grad(n + '/kernel'), self.grad(n + '/bias'))
            if n != 'conv2d':
                dx = self._dbuf('in:' + n, x)
                prev_is_plain_relu = inputs[n] in ('conv2d_2', 'conv2d_3')     # no pool between: fuse its ReluGrad
                ops.conv2d_bwd_data(self.desc[n], dzc, self.var(n + '/kernel'), dx,
                                    relu_mask=x if prev_is_plain_relu else None)
                d = dx


def fcsp_receptive():
    """(c0, jump) of the last pooled map of the unary conv stack over a whole image, in pixel indices: cell i sees the
    image through a window centred on c0 + i * jump.  Walked from DCNF_CONVS / DCNF_POOL_AFTER (VALID, stride 1; 2x2
    pools): a k x k conv moves the first centre by (k - 1) / 2 cells of its input, a pool by half a cell and doubles the
    jump.  Returned as (twice c0, jump), both integers: (49, 8) for the reference's stack, c0 = 24.5."""
    c0x2, jump = 0, 1
    for n, _, _, k in DCNF_CONVS:
        c0x2 += (k - 1) * jump
        if n in DCNF_POOL_AFTER:
            c0x2 += jump
            jump *= 2
    return c0x2, jump


def fcsp_maps(H, W, h, w, align='centre'):
    """The pixel-to-cell tables of superpixel pooling (ops.FcspMap): (ymap [H], xmap [W]) int32.
    'centre': a pixel belongs to the cell whose receptive-field centre is nearest,
    clamp(floor((2 y - 2 c0 + jump) / (2 jump)), 0, h - 1) in integers (fcsp_receptive); the model's choice.
    'nearest': min(y * h // H, h - 1), nearest-neighbour upsampling of the map to the image, the paper's; for a padded
    network the two coincide, for the reference's VALID convs 'nearest' is off by whole cells."""
    if align == 'centre':
        c0x2, jump = fcsp_receptive()

        def table(size, cells):
            y = np.arange(size, dtype=np.int64)
            return np.clip((2 * y - c0x2 + jump) // (2 * jump), 0, cells - 1).astype(np.int32)
    elif align == 'nearest':
        def table(size, cells):
            y = np.arange(size, dtype=np.int64)
            return np.minimum(y * cells // size, cells - 1).astype(np.int32)
    else:
        raise ValueError(f"fcsp_maps: align {align!r} is neither 'centre' nor 'nearest'")
    if min(H, W, h, w) <= 0:
        raise ValueError(f'fcsp_maps: image {H} x {W}, map {h} x {w}')
    return table(H, h), table(W, w)


class DCNFUnaryFCSP(DCNFUnary):
    """NON-REFERENCE (--unary fcsp): the unary part as Liu et al. 2015 build it in DCNF-FCSP.  The reference's five convs
    (the same names, shapes, VALID padding, ReLU and pools) run ONCE over the whole resized image instead of over 48
    overlapping patches; the last pooled map ([B,24,34,256] at 240x320) is averaged inside every superpixel
    (ops.superpixel_pool_fwd, include/a3d_fcsp.h: each pixel belongs to the cell whose receptive-field centre is nearest,
    fcsp_maps) and the [B * S, 256] rows go through the reference's three dense layers.  Only dense/kernel changes shape,
    [256,128] for [12544,128]; the parameters come from the same stream in the same order, so at equal seed the conv
    kernels are DCNFUnary's bits.  Offers what DCNFReplica uses of DCNFUnary; P is the number of dense rows, B * S.
    image_hw, sp, fuse_pool: for tests (DCNFReplica runs at 240x320, 40, fused).
    labels, label_count (None by default): a label map [B,H,W] and counts [B,S] int32 that DCNFReplica(segmentation='slic')
    attaches; the pooling and its transpose then run over the superpixels of that map (ops.label_pool_fwd / _bwd,
    include/a3d_slic.h) and read what the two tensors hold at the time of the launch."""

    def __init__(self, batchsize, device='cuda', params=None, seed=3000, precision='fp32',
                 image_hw=(DCNF_IMG_H, DCNF_IMG_W), sp=DCNF_SP, fuse_pool=None):
        H, W = (int(v) for v in image_hw)
        sp = int(sp)
        if sp <= 0 or H <= 0 or W <= 0 or H % sp or W % sp:
            raise ValueError(f'DCNFUnaryFCSP: image {H} x {W} is not cut into superpixels of edge {sp}')
        self.B = batchsize
        self.device = dev = torch.device(device)
        self.H, self.W, self.sp = H, W, sp
        self.rows, self.cols = H // sp, W // sp
        self.S = S = self.rows * self.cols
        self.P = P = batchsize * S
        shapes = collections.OrderedDict()
        for n, ci, co, k in DCNF_CONVS:
            shapes[DCNF_PREFIX + n + '/kernel'] = (k, k, ci, co)
            shapes[DCNF_PREFIX + n + '/bias'] = (co,)
        feat = DCNF_CONVS[-1][2]
        for n, i, o, _ in DCNF_DENSES:
            shapes[DCNF_PREFIX + n + '/kernel'] = (feat if n == 'dense' else i, o)
            shapes[DCNF_PREFIX + n + '/bias'] = (o,)
        self.shapes = shapes
        self.group = ParamGroup('unary', 0.1, shapes, dev, slots=False)    # GradientDescentOptimizer(0.1), src/models.py:198
        if params is None:
            rng = np.random.default_rng(seed)
            params = {n: (glorot_uniform(rng, s) if n.endswith('/kernel') else np.zeros(s, np.float32))
                      for n, s in shapes.items()}
        for n, s in shapes.items():
            if tuple(np.shape(params[n])) != tuple(s):
                raise ValueError(f'DCNFUnaryFCSP: {n} has shape {list(np.shape(params[n]))}, this form\'s is {list(s)}')
            self.group.view(self.group.var, n).copy_(torch.from_numpy(np.ascontiguousarray(params[n], np.float32)))

        def buf(*shape):
            return torch.empty(shape, device=dev)
        self.resized = buf(batchsize, H, W, 3)
        self.act = collections.OrderedDict()
        self.dact = {}
        self.desc = {}
        # as DCNFUnary: conv + ReLU + max pool in one kernel (fp32); fuse_pool=False keeps the pre-pool maps, for tests
        self.fuse_pool = precision == 'fp32' if fuse_pool is None else bool(fuse_pool) and precision == 'fp32'
        self.argmax, self.conv_hw = {}, {}
        self.act['x'] = self.resized
        h, w = H, W
        for n, ci, co, k in DCNF_CONVS:
            if h < k or w < k:
                raise ValueError(f'DCNFUnaryFCSP: image {H} x {W} is too small for {n}')
            self.desc[n] = ops.conv_desc(batchsize, h, w, ci, co, k, k, 1, 'VALID', precision=precision)
            h, w = h - k + 1, w - k + 1
            self.conv_hw[n] = (h, w)
            if not (self.fuse_pool and n in DCNF_POOL_AFTER):
                self.act[n] = buf(batchsize, h, w, co)
            if n in DCNF_POOL_AFTER:
                h, w = h // 2, w // 2                     # an odd last row / column is dropped, as the pool's ABI states
                if h == 0 or w == 0:
                    raise ValueError(f'DCNFUnaryFCSP: image {H} x {W} is too small for {n}\'s pool')
                self.act[n + '/pool'] = buf(batchsize, h, w, co)
                if self.fuse_pool:
                    self.argmax[n] = torch.empty((batchsize, h, w, co), dtype=torch.uint8, device=dev)
        self.map_hw = (h, w)
        self.map = ops.FcspMap(*fcsp_maps(H, W, h, w, 'centre'), h, w, sp, device=dev)
        self.labels = self.label_count = None       # DCNFReplica(segmentation='slic') attaches its label map and counts
        self.act['pooled'] = buf(P, feat)
        for n, i, o, _ in DCNF_DENSES:
            self.act[n] = buf(P, o)
        self.z = self.act['dense_2']
        self.few_pooled = (self.fuse_pool and dev.type == 'cuda'
                           and ops.conv2d_bwd_filter_pooled_supported(self.desc['conv2d']))

    def forward_resized(self, record_argmax=True):
        """The stack over self.resized as it stands (see DCNFUnary.forward_resized)."""
        t = self._forward_convs(self.resized, record_argmax)
        pooled = self.act['pooled'].view(self.B, self.S, -1)
        if self.labels is None:
            ops.superpixel_pool_fwd(t, self.map, pooled)
        else:
            ops.label_pool_fwd(t, self.map, self.labels, self.label_count, pooled)
        self._forward_denses(self.act['pooled'])
        return self.z.view(self.B, self.S, 1)

    def backward(self, dz):
        """Gradients of sum(z * dz) wrt every unary variable, into the flat gradient buffer."""
        a = self.act
        d0 = self._backward_denses(a['pooled'], dz)
        dpooled = self._dbuf('pooled', a['pooled'])
        ops.dense_bwd_data(d0, self.var('dense/kernel'), dpooled)
        dflat = self._dbuf('flat', a['conv2d_4/pool'])
        if self.labels is None:
            ops.superpixel_pool_bwd(dpooled.view(self.B, self.S, -1), self.map, dflat)     # writes every element
        else:
            ops.label_pool_bwd(dpooled.view(self.B, self.S, -1), self.map, self.labels, self.label_count, dflat)
        self._backward_convs(dflat)

    def load_convs_from(self, state):
        """Warm start from a checkpoint of the patch form (or of this one): copies the five convs' kernels and biases
        from a name -> tensor / array mapping and leaves the dense head as it is.  Returns the names copied."""
        names = [DCNF_PREFIX + n + suffix for n, _, _, _ in DCNF_CONVS for suffix in ('/kernel', '/bias')]
        for n in names:
            if n not in state or tuple(np.shape(state[n])) != tuple(self.shapes[n]):
                raise ValueError(f'load_convs_from: {n} is missing or not of shape {list(self.shapes[n])}')
        for n in names:
            v = state[n]
            v = v.detach() if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v, np.float32))
            self.group.view(self.group.var, n).copy_(v)
        return names


DCNF_GAMMA, DCNF_EPSILON = 1.0, 1e-7    # src/models.py:17-18
DCNF_PAIR_PREFIX = 'pairwise/pairwise_layers/dense/'


DCNF_SUPERPIXELS = (40, 20, 10)         # --superpixel: 6 x 8, 12 x 16, 24 x 32 superpixels on 240 x 320


def check_dcnf_superpixel(superpixel, unary, valid_range):
    """ValueError unless DCNFReplica can run at this superpixel edge with this unary form and these targets (the driver
    and the evaluation call it before any GPU work)."""
    if superpixel not in DCNF_SUPERPIXELS:
        raise ValueError(f'superpixel {superpixel!r}: one of {DCNF_SUPERPIXELS} (--superpixel)')
    if superpixel == DCNF_SP:
        return
    rows, cols = DCNF_IMG_H // superpixel, DCNF_IMG_W // superpixel
    if unary != 'fcsp':
        raise ValueError(f'superpixel {superpixel} needs --unary fcsp: the patch form would run {rows * cols} patches per '
                         f'image')
    if valid_range is not None:
        raise ValueError(f'superpixel {superpixel} cannot go with --min-depth / --max-depth yet: the likelihood of the '
                         f'observed superpixels alone exists only for the dense 6 x 8 CRF (--superpixel 40); on the banded '
                         f'CRF it is a later change')


DCNF_SEGMENTATIONS = ('grid', 'slic')    # --segmentation
DCNF_SLIC_ITERS, DCNF_SLIC_COMPACTNESS = 5, 0.1


def check_dcnf_segmentation(segmentation, unary, pairwise_texture, valid_range, slic_iters=DCNF_SLIC_ITERS,
                            slic_compactness=DCNF_SLIC_COMPACTNESS):
    """ValueError unless DCNFReplica can run on this segmentation with this unary form, these similarities and these
    targets (the drivers call it before any GPU work)."""
    if segmentation not in DCNF_SEGMENTATIONS:
        raise ValueError(f'segmentation {segmentation!r}: one of {DCNF_SEGMENTATIONS} (--segmentation)')
    if segmentation == 'grid':
        return
    if unary != 'fcsp':
        raise ValueError('--segmentation slic needs --unary fcsp: a patch is a square around a grid block, not a '
                         'superpixel of a label map')
    if pairwise_texture:
        raise ValueError('--segmentation slic cannot go with --pairwise-texture yet: the LBP histogram over the pixels of a '
                         'label map is a later change')
    if valid_range is not None:
        raise ValueError('--segmentation slic cannot go with --min-depth / --max-depth yet: the mean over the measured '
                         'pixels of a label map is a later change')
    if int(slic_iters) != slic_iters or slic_iters < 0:
        raise ValueError(f'--slic-iters {slic_iters!r}: a non-negative integer')
    if not 0 <= float(slic_compactness) < float('inf'):
        raise ValueError(f'--slic-compactness {slic_compactness!r}: a finite number >= 0')


def dcnf_pair_indices(rows, cols):
    """src/models.py:20-30: every interior superpixel on one colour of the checkerboard, paired with its four
    neighbours (up, down, left, right): two int lists (left, right)."""
    left, right = [], []
    for row in range(1, rows - 1):
        for col in range(2 - (row & 1), cols - 1, 2):
            pixel = row * cols + col
            for addend in (-cols, cols, -1, 1):
                left.append(pixel)
                right.append(pixel + addend)
    return left, right


class DCNFReplica(Replica):
    """The whole DCNF train step (src/models.py:179-200): resize to 240x320, unary z over 48 patches, pairwise r over 48
    superpixel pairs, CRF negative log-likelihood, gradient descent (0.1) on what receives a gradient.

    TF-1.3 semantics assumed (the oracle states the same, oracle/dcnf.py): scatter_nd_update has no gradient, so the CRF
    matrix A is a constant for the optimizer — the pairwise dense layer never moves and only the unary stack trains.

    train_pairwise (NON-REFERENCE, --train-pairwise): the pairwise dense layer learns too, as in Liu et al. 2015
    (eq. 9-14).  The loss launch also writes d loss / d r through A^-1 and log|A| (ops.crf_loss_grad: the same loss and
    dz bits), ops.pair_dense_bwd takes it to the layer's kernel and bias, and the `pairwise` group descends at its
    learning rate under the projection onto kernel, bias >= 0 (ops.sgd_apply_floor), which construction applies once
    to the initial values.  The unary group's step is the bits it would be without the flag, given the same pairwise
    values.  Off (the default), no launch and no buffer of the step differs from the reference form.

    pairwise_texture (NON-REFERENCE, --pairwise-texture): the paper's third pairwise observation, texture disparity over
    local-binary-pattern histograms (include/a3d_texture.h).  The dense layer's kernel is [3,1] under the same variable
    name, drawn from the same stream; the forward launches ops.superpixel_lbp_hist and ops.pair_similarity3 in place of
    ops.pair_similarity.  Meant to go with train_pairwise (the backward reads K from sims); without it the layer keeps
    its draw.  A [2,1] kernel is refused at restore, as a [3,1] one is without the argument.  Off (the default),
    construction and every launch are what they are without it.

    valid_range (NON-REFERENCE, --min-depth / --max-depth): (min_depth, max_depth) — the depth maps have holes
    (include/a3d_crf_valid.h).  The target is resized validity-aware (ops.resize_bilinear_tf1_valid: NaN where a tap is
    not finite or not in (min_depth, max_depth]), a superpixel's target is the mean of its measured pixels
    (ops.superpixel_mean_valid), and the objective is the field's negative log-likelihood of the observed superpixels
    alone, the others integrated out (ops.crf_loss_observed: no epsilons; with every superpixel observed it is the
    reference's loss without its three).  Its dz goes into the unary backward, its dr, under train_pairwise, into the
    pairwise layer's.  min_valid: a superpixel is a target only if at least ceil(min_valid * 40 * 40) of its pixels were
    measured.  The default, 0.5, is a choice, not a derivation: a mean over the measured minority of a block that is
    mostly sky or shadow describes its edge, not the superpixel.  None (the default): no launch, buffer or bit differs.

    unary (NON-REFERENCE, --unary fcsp): 'fcsp' takes z from DCNFUnaryFCSP, the convs once over the whole image and
    superpixel pooling before the dense head (Liu et al. 2015, DCNF-FCSP), in place of the 48 patches per image.  The rest
    of the step reads only z and the resized image and is the same code.  dense/kernel is [256,128] in that form and
    [12544,128] in the other; a restore across the two is refused.  'patch' (the default): no launch, buffer or bit
    differs.

    superpixel (NON-REFERENCE, --superpixel): the edge of the square superpixels, 40 (the reference's 6 x 8 grid of 48),
    20 (12 x 16 = 192) or 10 (24 x 32 = 768).  Every part of the step that reads a superpixel uses this replica's sp;
    no weight depends on it, so a checkpoint trained at one grid loads and evaluates at another.  20 and 10 need
    unary='fcsp' (the patch form would run 192 or 768 patches per image) and valid_range=None (the likelihood of the
    observed superpixels on a band is not built yet).  At 20 and 10 the CRF is the banded one (include/a3d_crf_band.h):
    forward_crf and nll launch ops.crf_band_nll (with dr iff train_pairwise), predict launches ops.crf_band_map, and
    self.status keeps its meaning.  The objective there is the field's negative log-likelihood WITHOUT the reference's
    three epsilons, e^T A e - log det A / 2 + S log(pi) / 2: the reference's form multiplies by pi^(S/2), which has no
    float32 value from S = 156.  Its value is not comparable with the --superpixel 40 loss.  The likelihood exists only for
    a positive definite A, so at 20 and 10 construction projects the pairwise kernel and bias onto >= 0 whether or not
    they train (r >= 0 makes A strictly diagonally dominant, every pivot >= 1).  40 (the default): today's code path,
    launches, buffers and bits.

    segmentation (NON-REFERENCE, --segmentation slic): 'slic' runs the field over SLIC superpixels of the resized image
    instead of square blocks (include/a3d_slic.h), the over-segmentation Liu et al. 2015 define DCNF on.  A pixel may only
    join one of the 3 x 3 clusters around its home block, so superpixel (R, C) stays within the blocks (R +- 1, C +- 1)
    and the pair graph, the CRF kernels and the band are the grid's, at all three --superpixel values.  Right after the
    resize, step, forward, predict and nll segment unary.resized (ops.slic_segment -> self.labels [B,240,320] int32,
    self.centres, self.label_count); the unary pools its last map over the labels (ops.label_pool_fwd / _bwd), y is
    ops.label_mean of the resized depth map, and r comes from the paper's similarities, the distance of the mean colours
    and of the frequency histograms, both in (0, 1] (ops.label_mean, ops.label_hist, ops.label_pair_similarity); the
    reference's grid similarities compare two blocks pixel by pixel and have no meaning for two shapes.  Everything else
    (pairs, loss, MAP, train_pairwise, descent, reducer, checkpoints, variable names and shapes) is the same code, and no
    weight depends on the segmentation: a checkpoint trained on one evaluates on the other.  predict() still returns
    [B, rows, cols]; depth_map() paints such values onto the pixels.  slic_iters = 5 and slic_compactness = 0.1 (in units
    of the [0, 1] RGB range) are choices, not derivations: few iterations move most of what will move, and 0.1 lets an edge
    of a tenth of the colour range outweigh a block's width.  RGB, not CIELAB, and no connectivity post-pass: the
    statistics do not need connected superpixels.  Needs unary='fcsp', no pairwise_texture, no valid_range; posterior()
    is refused.  'grid' (the default): no launch, buffer, bit, message or refusal differs.

    clip_norm (NON-REFERENCE, --clip-norm; include/a3d_clip.h): a number > 0, inf allowed.  The `unary` group's descent, and
    under train_pairwise the `pairwise` group's floored one, each bounded by its own gradient's global norm (the reduced
    gradient's under a reducer) through a control block of its own (ParamGroup.apply_sgd): the rate becomes fl32(lr * scale),
    and a step whose gradient is not finite moves nothing of that group.  One place in step(): every unary form passes
    through it.  None (the default): no launch, buffer or bit differs."""
    uses_dropout = False
    clip_norm = None

    def __init__(self, batchsize, device='cuda', params=None, seed=3000, global_step=0, reducer=None,
                 precision='fp32', train_pairwise=False, pairwise_texture=False, valid_range=None, min_valid=0.5,
                 unary='patch', superpixel=DCNF_SP, segmentation='grid', slic_iters=DCNF_SLIC_ITERS,
                 slic_compactness=DCNF_SLIC_COMPACTNESS, clip_norm=None):
        if unary not in ('patch', 'fcsp'):
            raise ValueError(f"unary {unary!r}: 'patch' or 'fcsp'")
        self.unary_form = unary
        check_dcnf_segmentation(segmentation, unary, pairwise_texture, valid_range, slic_iters, slic_compactness)
        self.slic = segmentation == 'slic'
        self.segmentation, self.slic_iters, self.slic_compactness = segmentation, int(slic_iters), float(slic_compactness)
        check_dcnf_superpixel(superpixel, unary, valid_range)
        self.sp = sp = int(superpixel)
        self.banded = sp != DCNF_SP
        valid_range = check_valid_range(valid_range)
        if not 0 <= float(min_valid) <= 1:
            raise ValueError(f'min_valid {min_valid!r}: the share of a superpixel that must be measured, 0 .. 1')
        self.valid_range, self.min_valid = valid_range, float(min_valid)
        self.min_count = int(math.ceil(self.min_valid * sp * sp))
        self.t_one = self.count = self.nobs = None      # allocated by the first launch that has holes to look for
        self.B = batchsize
        self.device = dev = torch.device(device)
        self.reducer = reducer
        self.train_pairwise = bool(train_pairwise)
        self.pairwise_texture = bool(pairwise_texture)
        self.nsims = 3 if self.pairwise_texture else 2
        self.global_step = global_step
        if params is not None:
            self._check_unary_kernel(np.shape(params[DCNF_PREFIX + 'dense/kernel']), 'params')
        if unary == 'fcsp':
            self.unary = DCNFUnaryFCSP(batchsize, dev, params=params, seed=seed, precision=precision, sp=sp)
        else:
            self.unary = DCNFUnary(batchsize, dev, params=params, seed=seed, precision=precision)
        self.rows, self.cols = DCNF_IMG_H // sp, DCNF_IMG_W // sp
        assert (self.rows, self.cols) == (self.unary.rows, self.unary.cols)
        self.nsp = self.rows * self.cols
        left, right = dcnf_pair_indices(self.rows, self.cols)
        self.left = torch.tensor(left, dtype=torch.int32, device=dev)
        self.right = torch.tensor(right, dtype=torch.int32, device=dev)
        self.band = ops.pair_band(left, right)
        pshapes = collections.OrderedDict([(DCNF_PAIR_PREFIX + 'kernel', (self.nsims, 1)), (DCNF_PAIR_PREFIX + 'bias', (1,))])
        if clip_norm is not None:
            self.clip_norm = check_clip_norm(clip_norm)
        self.pair_group = ParamGroup('pairwise', 0.1, pshapes, dev, slots=False,
                                     clip_norm=self.clip_norm if self.train_pairwise else None)
        if params is None or DCNF_PAIR_PREFIX + 'kernel' not in params:
            rng = np.random.default_rng(seed + 1)
            pw = {DCNF_PAIR_PREFIX + 'kernel': glorot_uniform(rng, (self.nsims, 1)),
                  DCNF_PAIR_PREFIX + 'bias': np.zeros((1,), np.float32)}
        else:
            pw = params
            self._check_pair_kernel(np.shape(pw[DCNF_PAIR_PREFIX + 'kernel']), 'params')
        for n in pshapes:
            self.pair_group.view(self.pair_group.var, n).copy_(
                torch.from_numpy(np.ascontiguousarray(pw[n], np.float32)))
        if self.train_pairwise or self.banded:
            ops.sgd_apply_floor(self.pair_group.var, self.pair_group.grad, 0.0, 0.0)      # beta >= 0 from the start
        if self.clip_norm is not None:      # the unary stack builds its group itself: the control block is given here
            g = self.unary.group
            g.clip_norm, g.ctl, g.ws = self.clip_norm, ops.clip_ctl(dev), ops.grad_norm_ws(g.count, dev)
        self.groups = collections.OrderedDict([('unary', self.unary.group), ('pairwise', self.pair_group)])
        self.depths240 = torch.empty((batchsize, DCNF_IMG_H, DCNF_IMG_W, 1), device=dev)
        self.hist = torch.empty((batchsize, self.nsp, 256), device=dev)
        if self.pairwise_texture:
            self.lbp = torch.empty((batchsize, self.nsp, 256), device=dev)
        self.y = torch.empty((batchsize, self.nsp, 1), device=dev)
        self.output = torch.empty((batchsize, DCNF_IMG_H, DCNF_IMG_W, 1), device=dev)
        self.sims = self.r = self.loss = self.loss_per_image = self.dz = self.dr = None
        self.crf = torch.empty((batchsize, self.nsp), device=dev)                          # predict(): the MAP depths
        self.status = torch.zeros((batchsize,), dtype=torch.int32, device=dev)    # the dense 6 x 8 step never writes it
        self.labels = None
        if self.slic:
            self.labels = torch.empty((batchsize, DCNF_IMG_H, DCNF_IMG_W), dtype=torch.int32, device=dev)
            self.centres = torch.empty((batchsize, self.nsp, 5), device=dev)
            self.label_count = torch.empty((batchsize, self.nsp), dtype=torch.int32, device=dev)
            self.mean3 = torch.empty((batchsize, self.nsp, 3), device=dev)
            self.count3 = torch.empty((batchsize, self.nsp), dtype=torch.int32, device=dev)
            self.unary.labels, self.unary.label_count = self.labels, self.label_count

    def pair_var(self, name):
        return self.pair_group.view(self.pair_group.var, DCNF_PAIR_PREFIX + name)

    def pair_grad(self, name):
        return self.pair_group.view(self.pair_group.grad, DCNF_PAIR_PREFIX + name)

    def _check_pair_kernel(self, shape, what):
        """The pairwise kernel about to be restored has this replica's number of similarities, or ValueError."""
        want = (self.nsims, 1)
        if tuple(shape) != want:
            raise ValueError(f'{what}: {DCNF_PAIR_PREFIX}kernel has shape {list(shape)}, this replica\'s is {list(want)} '
                             f'(pairwise_texture={self.pairwise_texture}: [3, 1] with --pairwise-texture, [2, 1] without)')

    def _check_unary_kernel(self, shape, what):
        """The unary dense/kernel about to be restored is of this replica's form, or ValueError."""
        want = (DCNF_CONVS[-1][2] if self.unary_form == 'fcsp' else DCNF_DENSES[0][1], DCNF_DENSES[0][2])
        if tuple(shape) != want:
            raise ValueError(f'{what}: {DCNF_PREFIX}dense/kernel has shape {list(shape)}, this replica\'s is {list(want)} '
                             f'(unary={self.unary_form!r}: [256, 128] with --unary fcsp, [12544, 128] with --unary patch)')

    def _pairwise(self):
        """The similarities of every pair and the pair weights r from the resized images (src/models.py:112-127)."""
        x = self.unary.resized
        if self.slic:
            ops.label_mean(x, self.sp, self.labels, self.mean3, self.count3)
            ops.label_hist(x, self.sp, self.labels, self.hist)
            self.sims, self.r = ops.label_pair_similarity(self.mean3, self.hist, self.label_count, self.left, self.right,
                                                          self.pair_var('kernel'), self.pair_var('bias'), DCNF_GAMMA)
            return
        ops.superpixel_hist(x, self.sp, self.hist)                                        # :112-113
        kernel, bias = self.pair_var('kernel'), self.pair_var('bias')
        if self.pairwise_texture:
            ops.superpixel_lbp_hist(x, self.sp, self.lbp)
            self.sims, self.r = ops.pair_similarity3(x, self.sp, self.hist, self.lbp, self.left, self.right, kernel, bias,
                                                     DCNF_GAMMA)
        else:
            self.sims, self.r = ops.pair_similarity(x, self.sp, self.hist, self.left, self.right, kernel, bias,
                                                    DCNF_GAMMA)                           # :115-127

    def forward(self, images, depths):
        """z, r and the loss; leaves d loss / d z in self.dz."""
        if self.slic:
            ops.resize_bilinear_tf1(images, self.unary.resized)                           # unary.forward's first launch
            self._segment()
            self.unary.forward_resized()
        else:
            self.unary.forward(images)                                                    # src/models.py:180,183
        return self.forward_crf(depths)

    def _segment(self):
        """SLIC superpixels of unary.resized as it stands, into self.labels, self.centres and self.label_count."""
        ops.slic_segment(self.unary.resized, self.sp, self.slic_iters, self.slic_compactness, self.labels, self.centres,
                         self.label_count)

    def depth_map(self, values):
        """Per-superpixel values [B, rows, cols] (or [B, nsp]) painted onto the pixels -> [B, 240, 320]: every pixel gets
        the value of its superpixel, by the labels of the last forward under segmentation='slic', by the blocks otherwise."""
        values = values.reshape(self.B, self.nsp)
        if self.slic:
            return ops.paint_labels(values, self.labels)
        return values.view(self.B, self.rows, 1, self.cols, 1).expand(-1, -1, self.sp, -1, self.sp).reshape(
            self.B, DCNF_IMG_H, DCNF_IMG_W)

    def forward_crf(self, depths):
        """Everything after the unary stack: target superpixels, pairwise r, CRF loss and d loss / d z."""
        self._targets(depths, self.B, self.valid_range)
        self._pairwise()
        self.loss, self.loss_per_image, self.dz, self.dr = self._objective(self.B, self.valid_range, self.train_pairwise)
        return self.loss

    def _targets(self, depths, n, valid_range):
        """The target superpixels of rows [0, n) into self.y: the means over the resized depth maps' blocks
        (src/models.py:181,131-132); with valid_range through the validity-aware resize and mean, NaN where a superpixel
        is no target, the numbers of measured pixels in self.count."""
        if valid_range is None:
            ops.resize_bilinear_tf1(depths[:n], self.depths240[:n])
            if self.slic:
                ops.label_mean(self.depths240[:n], self.sp, self.labels[:n], self.y[:n], self.count3[:n])
            else:
                ops.superpixel_mean(self.depths240[:n], self.sp, self.y[:n])
            return
        if self.t_one is None:
            self.t_one = torch.empty((self.B, 1, 1, 1), device=self.device)
            self.count = torch.empty((self.B, self.nsp), dtype=torch.int32, device=self.device)
        lo, hi = valid_range
        ops.resize_bilinear_tf1_valid(depths[:n], self.depths240[:n], lo, hi, scratch=self.t_one[:n])
        ops.superpixel_mean_valid(self.depths240[:n], self.sp, self.min_count, out=self.y.view(self.B, self.nsp)[:n],
                                  count=self.count[:n])

    def _objective(self, n, valid_range, pair_grad):
        """The objective on rows [0, n) of the z, y and r that stand in the buffers, in one launch: (mean [1], per image,
        dz, dr or None without pair_grad).  With valid_range the likelihood of the observed superpixels, which leaves
        self.nobs and self.status_observed; on the banded CRF its likelihood, which leaves those rows of self.status;
        else the reference's loss (src/models.py:129-177)."""
        args = (self.unary.z.view(self.B, self.nsp)[:n], self.y.view(self.B, self.nsp)[:n], self.r[:n], self.left, self.right)
        if valid_range is not None:
            mean, per, dz, dr, self.nobs, self.status_observed = ops.crf_loss_observed(*args, pair_grad=pair_grad)
        elif self.banded:
            mean, per, dz, dr, _, status = ops.crf_band_nll(*args, self.band, pair_grad=pair_grad)
            self.status[:n].copy_(status)
        elif pair_grad:
            mean, per, dz, dr = ops.crf_loss_grad(*args, DCNF_EPSILON)
        else:
            (mean, per, dz), dr = ops.crf_loss(*args, DCNF_EPSILON), None
        return mean, per, dz, dr

    def _predict_forward(self, images, n, who):
        """predict()'s network part: z of rows [0, n) of images (default all) and of zero images in rows n .. B, and the
        pair weights in self.r.  Returns n."""
        B, u = self.B, self.unary
        n = images.shape[0] if n is None else int(n)
        check_rows(who, n, B, f'a batch of {images.shape[0]} images', images.shape[0])
        ops.resize_bilinear_tf1(images[:n], u.resized[:n])                               # src/models.py:180
        if n < B:
            u.resized[n:].zero_()
        if self.slic:
            self._segment()
        u.forward_resized(record_argmax=False)
        self._pairwise()
        return n

    def predict(self, images, n=None):
        """The model's depths for a batch of images, without targets: (unary, crf), each [B, rows, cols] float32 (views
        of this replica's buffers, valid until its next forward).  unary is z, what the reference draws as `Output`
        (src/models.py:187-191); crf is the field's MAP estimate A^-1 z (ops.crf_map), which the reference never forms.
        images [m, H, W, 3] float32, or the uint8 pixel values of converter-written records, m <= B; only rows [0, n)
        (default m) are read, rows n .. B of the network input are zero, so a short last batch runs at the replica's B
        and its rows [0, n) are those of a full batch.  Leaves the pair weights in self.r and, per image, 1 in
        self.status where the system was singular (that row of crf is NaN).  Weights, gradients and global_step are
        left as they are."""
        B, u = self.B, self.unary
        self._predict_forward(images, n, 'predict')
        if self.banded:
            ops.crf_band_map(u.z.view(B, self.nsp), self.r, self.left, self.right, self.band, self.crf, self.status)
        else:
            self.crf, self.status = ops.crf_map(u.z.view(B, self.nsp), self.r, self.left, self.right, self.crf, self.status)
        return u.z.view(B, self.rows, self.cols), self.crf.view(B, self.rows, self.cols)

    def posterior(self, images, depths=None, n=None, valid_range=None, want_var=True, keep=None):
        """NON-REFERENCE (include/a3d_posterior.h): the field as a distribution at prediction -> (mean, var), each
        [B, rows, cols] float32 (var None without want_var; valid until the next call).  Runs predict()'s forward and pair
        weights (images None: the z and r that predict() or posterior() just left, n given), then ops.crf_band_posterior,
        at all three grids (6 x 8 is a band of 8) and for both unary forms.  Without
        depths mean is the MAP estimate (predict()'s crf on the banded grids, bit for bit) and var the field's marginal
        variance A^-1_ii / 2.  With depths [m, H, W, 1] the field is conditioned on the superpixels they measure: the
        targets of _targets(depths, n, valid_range), which needs valid_range = (min_depth, max_depth); mean is the target on
        a measured superpixel and the conditional mean elsewhere, var 0 and the conditional variance.  Leaves the numbers of
        measured superpixels in self.nobs and, per image, 1 in self.status where the system was not positive definite (NaN
        rows; at superpixel 40 the pair weights are not projected onto >= 0, and an indefinite A is no distribution).  Rows
        n .. B are those of a zero image without depths.  keep ([n, nsp] bool on the device, with depths): only the targets
        it marks are conditioned on, the others are hidden from the field; self.y keeps every target (NaN where the depth
        map measures none).  Training state, self.valid_range included, is left as it is."""
        B = self.B
        if self.slic:
            raise ValueError("posterior: not with segmentation='slic' yet (--segmentation slic): conditioning on the "
                             'measured pixels of a label map is a later change')
        if images is None and (self.r is None or n is None):
            raise ValueError('posterior: images None reuses the last predict(): call it first and pass n')
        n = images.shape[0] if n is None else int(n)
        m = B if images is None else images.shape[0]
        y = None
        if depths is not None:
            if valid_range is None:
                raise ValueError('posterior: depths need valid_range = (min_depth, max_depth), which says what a hole is')
            valid_range = check_valid_range(valid_range)
            check_rows('posterior', n, B, f'{m} images and {depths.shape[0]} depth maps', m, depths.shape[0])
        elif valid_range is not None or keep is not None:
            raise ValueError('posterior: valid_range or keep without depths')
        if keep is not None and (keep.dtype != torch.bool or tuple(keep.shape) != (n, self.nsp)):
            raise ValueError(f'posterior: keep {tuple(keep.shape)} {keep.dtype} must be bool {(n, self.nsp)}')
        if images is not None:
            self._predict_forward(images, n, 'posterior')
        elif not 0 < n <= B:
            raise ValueError(f'posterior: n = {n}, replica batch {B}')
        if depths is not None:
            self._targets(depths, n, valid_range)
            y = self.y.view(B, self.nsp)
            if n < B:
                y[n:].fill_(float('nan'))
            if keep is not None:
                y = y.clone()
                y[:n].masked_fill_(~keep, float('nan'))
        if getattr(self, 'post_mean', None) is None:
            self.post_mean = torch.empty((B, self.nsp), device=self.device)
            self.post_var = torch.empty((B, self.nsp), device=self.device)
        mean, var, self.nobs, status = ops.crf_band_posterior(
            self.unary.z.view(B, self.nsp), y, self.r, self.left, self.right, self.band, want_var=want_var,
            mean=self.post_mean, var=self.post_var if want_var else None)
        self.status.copy_(status)
        return mean.view(B, self.rows, self.cols), None if var is None else var.view(B, self.rows, self.cols)

    def nll(self, depths, n, valid_range=None):
        """The training objective (src/models.py:129-177) on rows [0, n) of the batch predict() just ran, from the z
        and r it left: the mean of the n images' CRF negative log-likelihoods, [1] float32 on the device.  valid_range
        (the replica's by default): the likelihood of the observed superpixels instead, as the train step computes it; the
        numbers of observed superpixels are left in self.nobs."""
        n = int(n)
        check_rows('nll', n, self.B, f'{depths.shape[0]} depth maps', depths.shape[0], ready=self.r is not None,
                   tail=', after predict()')
        valid_range = self.valid_range if valid_range is None else valid_range
        if valid_range is not None and self.slic:
            raise ValueError("nll: segmentation='slic' has no mean over the measured pixels of a label map yet (valid_range)")
        if valid_range is not None and self.banded:
            raise ValueError(f'nll: superpixel {self.sp} has no likelihood of observed superpixels alone yet (valid_range)')
        self._targets(depths, n, valid_range)
        return self._objective(n, valid_range, False)[0]

    def step(self, images, depths, keep_mask=None):
        self.forward(images, depths)
        self.unary.backward(self.dz)
        if self.train_pairwise:
            ops.pair_dense_bwd(self.sims, self.dr, self.pair_grad('kernel'), self.pair_grad('bias'))
        red = self.reducer
        scale = 1.0
        if red is not None:
            red.start(self.unary.group.grad)
            if self.train_pairwise:
                red.start(self.pair_group.grad)
            red.finish()
            scale = 1.0 / red.world_size
        self.unary.group.apply_sgd(scale)                                                 # :198-200
        if self.train_pairwise:
            self.pair_group.apply_sgd(scale, floor=0.0)
        self.global_step += 1
        return {'mean_loss': self.loss}

    def summary_scalars(self, out):
        rec = {'loss/mean_loss': float(out['mean_loss'])}                                 # src/models.py:174
        if self.valid_range is not None:                 # NON-REFERENCE: share of the superpixels that were targets
            rec['loss/observed_fraction'] = float(self.nobs.sum()) / (self.B * self.nsp)
        if self.clip_norm is not None:                   # NON-REFERENCE: the groups the step applies
            self.unary.group.clip_scalars(rec)
            if self.train_pairwise:
                self.pair_group.clip_scalars(rec)
        return rec

    def summary_images(self):
        """src/models.py:187-196; max_outputs=1."""
        ops.resize_bilinear_tf1(self.unary.z.view(self.B, self.rows, self.cols, 1), self.output)
        target = self.depths240 if self.valid_range is None else torch.nan_to_num(self.depths240[:1], nan=0.0)   # a hole is 0
        return [('summaries/Output', self.output, 1), ('summaries/Input', self.unary.resized, 1),
                ('summaries/Target', target, 1)]

    def broadcast_state(self, dist, src=0):
        for g in self.groups.values():
            dist.broadcast(g.var, src)
        self._broadcast_step(dist, src)

    def gather_state(self):
        """Nothing is sharded here (the driver calls this on every replica before a checkpoint)."""

    def state_dict(self):
        sd = collections.OrderedDict()
        for g in self.groups.values():
            for n in g.offsets:
                sd[n] = g.view(g.var, n)
        sd['global_step'] = torch.tensor(self.global_step, dtype=torch.int64)
        return sd

    def load_state_dict(self, sd):
        self._check_pair_kernel(sd[DCNF_PAIR_PREFIX + 'kernel'].shape, 'load_state_dict')
        self._check_unary_kernel(sd[DCNF_PREFIX + 'dense/kernel'].shape, 'load_state_dict')
        for g in self.groups.values():
            for n in g.offsets:
                g.view(g.var, n).copy_(sd[n])
        self.global_step = int(sd['global_step'].item())

    def load_tf_variables(self, tensors):
        """Restore from a TensorFlow checkpoint's whole tensors (the reference's dcnf partitions its variables, which
        tfckpt.read_bundle refuses; a bundle written by this build loads)."""
        self._check_pair_kernel(np.shape(tensors[DCNF_PAIR_PREFIX + 'kernel']), 'load_tf_variables')
        self._check_unary_kernel(np.shape(tensors[DCNF_PREFIX + 'dense/kernel']), 'load_tf_variables')
        for g in self.groups.values():
            for n in g.offsets:
                g.view(g.var, n).copy_(torch.from_numpy(np.ascontiguousarray(tensors[n], np.float32)))
        if 'global_step' in tensors:
            self.global_step = int(np.asarray(tensors['global_step']).reshape(-1)[0])


# =====================================================================================================
# plugin surface: models.msdn / models.dcnf  (src/models.py:370-371)
# =====================================================================================================
class TrainOp:
    """What `model(inputs, targets)` returns: run() is one `session.run(train_op)`.

    Input side: a feed.DeviceFeed over the shuffle queue; batch k+1 is in flight while step k computes.

    augment (NON-REFERENCE, an augment.Eigen2014): every batch is warped as it is resized.  Its table is drawn beside the
    batch's DMA for the global step that will consume it, from (seed, rank, step) alone, and travels under the same event."""

    def __init__(self, replica, pipeline, seed=0, augment=None, rank=0):
        self.replica, self.pipeline, self.seed = replica, pipeline, seed
        self.augment, self.rank = augment, rank
        dev = replica.device
        self.keep = torch.empty((replica.B, 4096), dtype=torch.uint8, device=dev) if replica.uses_dropout else None
        self.feed = DeviceFeed(pipeline, replica.B, dev)
        self.last = None
        if augment is not None:
            self.hw = tuple(self.feed.pool[0].shape[1:3])
            if self.hw != tuple(self.feed.pool[1].shape[1:3]):
                raise ValueError(f'augmentation warps the image and its depth map with one map: they must be stored at the '
                                 f'same size, not {self.hw} and {tuple(self.feed.pool[1].shape[1:3])}')
            self.table_host = [torch.empty((replica.B, augment_.STRIDE), dtype=torch.float32).pin_memory() for _ in range(2)]
            self.table_dev = [torch.empty((replica.B, augment_.STRIDE), device=dev) for _ in range(2)]
            self.table_step = [None, None]  # the global step table i was drawn for
        self.feed.start(self._draw)

    def _draw(self, i, j):
        """The feed's hook: batch j, just copied into buffer i, will be consumed j - k steps from now."""
        if self.augment is not None:
            self._table(i, self.replica.global_step + j - self.feed.k)

    def _table(self, i, step):
        """Draw the table of global step `step` into pinned buffer i and start its copy (the current stream is the copy
        stream; the earlier copy out of that buffer has finished: the feed waited for `copied` before releasing the slots)."""
        h, w = self.hw
        augment_.table(self.augment, self.seed, self.rank, step, self.replica.B, h, w, out=self.table_host[i].numpy())
        self.table_dev[i].copy_(self.table_host[i], non_blocking=True)
        self.table_step[i] = step

    def run(self):
        r, feed = self.replica, self.feed
        i = feed.k & 1
        if self.augment is not None and feed.due() is None and self.table_step[i] != r.global_step:
            # the batch was prefetched before a checkpoint moved global_step (the first two steps of a resumed run)
            feed.redo(i, lambda: self._table(i, r.global_step))
        images, depths, _, i = feed.take()
        if self.keep is not None:
            ops.dropout_keep_mask(self.keep, self.seed, r.global_step)
        if self.augment is None:
            self.last = r.step(images, depths, self.keep)
        else:
            self.last = r.step(images, depths, self.keep, warp=self.table_dev[i])
        feed.give_back(self._draw)
        return self.last

    @property
    def global_step(self):
        return self.replica.global_step


class _MultiScaleDeepNetwork:
    """Eigen et al. (2014) coarse+fine network — plugin wrapper around MSDNReplica (src/models.py:203-367)."""
    beta2 = 1.0          # the reference's AdamOptimizer(rate, momentum, 1): alpha == 0, weights never move
    reducer = None       # set by the driver when world_size > 1
    seed = 3000
    precision = 'fp32'   # --precision: 'fp32' | 'bf16x3' | 'bf16' (see MSDNReplica)
    augment = None       # NON-REFERENCE, --augment eigen: an augment.Eigen2014 (train-time augmentation of the input batch)
    valid_range = None   # NON-REFERENCE, --min-depth / --max-depth: (min, max), the depth maps have holes (see MSDNReplica)
    grad_weight = 0.0    # NON-REFERENCE, --loss-gradient: weight of the gradient-matching term in both losses (see MSDNReplica)
    objective = 'silog'  # NON-REFERENCE, --loss berhu / ssi: reverse Huber, or scale-and-shift-invariant (see MSDNReplica)
    berhu_fraction = 0.2  # --berhu-fraction: its threshold, as a fraction of each sample's largest error
    optimizer = 'adam'   # NON-REFERENCE, --optimizer momentum: SGD with momentum, the rule the rates were published for (see MSDNReplica)
    momentum = 0.9       # --momentum: its momentum
    lr_scale = 1.0       # NON-REFERENCE, --lr-scale: a factor on every rate of MSDN_OPTIMIZERS
    clip_norm = None     # NON-REFERENCE, --clip-norm: bound on every optimizer group's gradient norm (see MSDNReplica)

    def __call__(self, images, depths, train=True):
        assert images.pipeline is depths.pipeline, 'inputs and targets must come from the same data.inputs() call'
        self.train = train
        replica = MSDNReplica(images.pipeline.B, device=torch.device('cuda', torch.cuda.current_device()),
                              seed=self.seed, beta2=self.beta2, reducer=self.reducer, precision=self.precision,
                              keep_dense_grads=False,        # one GPU + the reference's optimizer: dW feeds ApplyAdam directly
                              valid_range=self.valid_range, grad_weight=self.grad_weight, objective=self.objective,
                              berhu_fraction=self.berhu_fraction, optimizer=self.optimizer, momentum=self.momentum,
                              lr_scale=self.lr_scale, clip_norm=self.clip_norm)
        replica.uses_dropout = bool(train)                   # train=False: tf.layers.dropout(training=False), src/models.py:230
        if self.reducer is not None:                         # replicas start from rank 0's weights
            for g in replica.groups.values():
                self.reducer.broadcast(g.var)
        rank = self.reducer.rank if self.reducer else 0
        return TrainOp(replica, images.pipeline, seed=self.seed + 1000 * rank, augment=self.augment if train else None,
                       rank=rank)


class _DistributedConvolutionalNeuralFields:
    """Liu et al. (2015) — plugin wrapper around DCNFReplica (src/models.py:13-200).  The reference pins its layers
    to /job:worker/task:{1,2,3} (src/models.py:63-79); here every replica holds the whole model and replicas are
    data-parallel, like msdn."""
    reducer = None
    seed = 3000
    precision = 'fp32'
    beta2 = None         # accepted for symmetry with msdn; gradient descent has no beta
    train_pairwise = False   # NON-REFERENCE, --train-pairwise: the pairwise dense layer learns, >= 0 (see DCNFReplica)
    pairwise_texture = False  # NON-REFERENCE, --pairwise-texture: LBP texture disparity as a third similarity (see DCNFReplica)
    valid_range = None   # NON-REFERENCE, --min-depth / --max-depth: (min, max), the depth maps have holes (see DCNFReplica)
    min_valid = 0.5      # the share of a superpixel that must be measured for it to be a target (see DCNFReplica)
    unary = 'patch'      # NON-REFERENCE, --unary fcsp: convs once over the image + superpixel pooling (see DCNFReplica)
    superpixel = DCNF_SP  # NON-REFERENCE, --superpixel 20 / 10: finer grids on the banded CRF (see DCNFReplica)
    segmentation = 'grid'  # NON-REFERENCE, --segmentation slic: SLIC superpixels in place of square blocks (see DCNFReplica)
    slic_iters, slic_compactness = DCNF_SLIC_ITERS, DCNF_SLIC_COMPACTNESS
    clip_norm = None     # NON-REFERENCE, --clip-norm: bound on every optimizer group's gradient norm (see DCNFReplica)

    def __call__(self, images, depths, train=True):
        assert images.pipeline is depths.pipeline, 'inputs and targets must come from the same data.inputs() call'
        self.train = train
        replica = DCNFReplica(images.pipeline.B, device=torch.device('cuda', torch.cuda.current_device()),
                              seed=self.seed, reducer=self.reducer, precision=self.precision,
                              train_pairwise=self.train_pairwise and train, pairwise_texture=self.pairwise_texture,
                              valid_range=self.valid_range, min_valid=self.min_valid, unary=self.unary,
                              superpixel=self.superpixel, segmentation=self.segmentation, slic_iters=self.slic_iters,
                              slic_compactness=self.slic_compactness, clip_norm=self.clip_norm if train else None)
        if self.reducer is not None:
            for g in replica.groups.values():
                self.reducer.broadcast(g.var)
        return TrainOp(replica, images.pipeline, seed=self.seed)


dcnf = _DistributedConvolutionalNeuralFields()
msdn = _MultiScaleDeepNetwork()
