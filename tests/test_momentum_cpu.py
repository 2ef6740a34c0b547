"""tests/momentum_ref.py, the host statement of SGD with momentum that the GPU tests hold the kernels and the replica to, pinned
against torch.optim.SGD(momentum=mu) on the CPU; and models.checkpoint_optimizer on literal key sets.  No GPU.

torch computes buf = mu buf + g and p = p - lr buf, possibly with a fused multiply-add.  At lr = 0.125, mu = 0.5 both products are
exact, so a fusion changes nothing and every bit agrees.  At the paper's rates the accumulator still agrees bit for bit (mu buf
is rounded before g is added on both sides); var may differ in its last bit wherever torch fuses lr buf into the subtraction."""
import numpy as np
import pytest
import torch

import momentum_ref as MR

COUNT, STEPS = 100003, 5


@pytest.mark.parametrize('lr,mu,var_ulps', [(0.125, 0.5, 0), (0.1, 0.9, 1), (0.001, 0.9, 1)])
def test_float32_restatement_is_torch_sgd_with_momentum(lr, mu, var_ulps):
    """Five steps.  The accumulator never sees var, so it is compared along the whole run.  var is compared step by step, each
    step of the restatement starting from torch's own var: the one difference a step can make is torch's fused lr buf, which
    saves the rounding of the product, at most half an ulp of it, before a subtraction that rounds once on either side: two
    reals that close round to the same float or to neighbours.  An ulp is that of the largest of the subtraction's operands and
    result, |var|, |lr buf| or |var'|: where the operands nearly cancel, the same absolute difference is many ulps of the small
    result, and it is the operands' grid that bounds it."""
    rng = np.random.default_rng(7)
    var = rng.standard_normal(COUNT).astype(np.float32)
    accum = np.zeros(COUNT, np.float32)
    p = torch.nn.Parameter(torch.from_numpy(var.copy()))
    opt = torch.optim.SGD([p], lr=lr, momentum=mu)
    for step in range(STEPS):
        g = rng.standard_normal(COUNT).astype(np.float32)
        before = p.detach().numpy().copy()
        var, accum = MR.step(before, accum, g, lr, mu)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        buf, after = opt.state[p]['momentum_buffer'].numpy(), p.detach().numpy()
        ulp = np.spacing(np.maximum.reduce([np.abs(before), np.abs(np.float32(lr) * accum), np.abs(var), np.abs(after)]))
        off = np.abs(var.astype(np.float64) - after) / ulp
        wrong_acc = int((accum.view(np.uint32) != buf.view(np.uint32)).sum())
        print(f'lr {lr} mu {mu} step {step}: accumulator {wrong_acc} mismatches, var {int((off != 0).sum())} ({(off != 0).mean():.1%}), '
              f'at most {off.max():.3g} ulp')
        assert wrong_acc == 0                          # torch's first step is buf = g, and 0 * mu + g is g
        assert off.max() <= var_ulps


def test_grad_scale_is_applied_to_the_gradient_first_and_skipped_at_one():
    rng = np.random.default_rng(8)
    var, accum, g = (rng.standard_normal(1000).astype(np.float32) for _ in range(3))
    third = np.float32(1 / 3)
    v1, a1 = MR.step(var, accum, g, 0.1, 0.9, 1 / 3)
    v2, a2 = MR.step(var, accum, g * third, 0.1, 0.9)
    assert np.array_equal(v1, v2) and np.array_equal(a1, a2) and not np.array_equal(a1, MR.step(var, accum, g, 0.1, 0.9)[1])
    assert v1.dtype == a1.dtype == np.float32
    # -0 * 1 would stay -0; the point of the skip is that the bits of g are not touched at all
    v, a = MR.step(np.zeros(1, np.float32), np.zeros(1, np.float32), np.array([np.nan], np.float32), 0.0, 0.0)
    assert np.isnan(v).all() and np.isnan(a).all()                           # 0 * NaN is NaN: lr = 0 does not protect var


def test_float64_form_agrees_where_every_operation_is_exact():
    rng = np.random.default_rng(9)
    var, accum, g = (rng.integers(-64, 65, 4096).astype(np.float32) for _ in range(3))
    v32, a32 = MR.step(var, accum, g, 0.25, 0.5, 0.5)
    v64, a64 = MR.step64(var, accum, g, 0.25, 0.5, 0.5)
    assert np.array_equal(v32.astype(np.float64), v64) and np.array_equal(a32.astype(np.float64), a64)


def test_checkpoint_optimizer_reads_the_slots():
    from ann3depth_amd import models
    var = 'coarse/conv/conv2d_0/kernel'
    weights = {var: 0, 'fine/third/bias': 0, 'global_step': 0}
    adam = dict(weights, **{var + '/CoarseConv': 0, var + '/CoarseConv_1': 0, 'fine/third/bias/FineA': 0, 'fine/third/bias/FineA_1': 0,
                            'CoarseConv/beta1_power': 0, 'CoarseConv/beta2_power': 0})
    bundle = dict(weights, **{var + '/CoarseConv': 0, 'fine/third/bias/FineA': 0})
    assert models.checkpoint_optimizer(adam) == 'adam'
    assert models.checkpoint_optimizer(dict(bundle, optimizer='momentum')) == 'momentum'       # a .pt state says so
    assert models.checkpoint_optimizer(bundle) == 'momentum'                                   # a bundle carries no string
    assert models.checkpoint_optimizer(weights) == 'adam'                                      # weights only
    assert models.checkpoint_optimizer({}) == 'adam'
    # some of Adam's first slots and none of its second (a partial TensorFlow checkpoint): still Adam's
    assert models.checkpoint_optimizer(dict(weights, **{var + '/CoarseConv': 0})) == 'adam'
    assert models.checkpoint_optimizer(dict(adam, optimizer='adam')) == 'adam'
    assert models.MSDN_OPTIMIZER_RULES == ('adam', 'momentum')
    assert models.msdn.optimizer == 'adam' and models.msdn.momentum == 0.9 and models.msdn.lr_scale == 1.0


def test_the_flags_are_listed_as_non_reference(capsys):
    from ann3depth_amd import ann3depth
    with pytest.raises(SystemExit):
        ann3depth.parse_args(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    for flag in ('--optimizer {adam,momentum}', '--momentum M', '--lr-scale S'):
        assert flag in text, flag
        assert text.split(flag)[-1].lstrip().startswith('NON-REFERENCE'), flag
    args = ann3depth.parse_args(['nyu'])
    assert args.optimizer == 'adam' and args.momentum is None and args.lr_scale is None
