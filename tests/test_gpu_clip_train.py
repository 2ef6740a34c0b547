"""The training steps and the driver under gradient clipping by global norm (MSDNReplica(clip_norm=), DCNFReplica(clip_norm=),
--clip-norm; include/a3d_clip.h).  Without the argument a replica is today's, bit for bit; with inf it is the unfused, unclipped
one; below the measured norms every applied group goes by its own rule at its own scale read back from the device, that scale
within one float32 ulp of tests/clip_ref.py on the replica's own gradient; a group whose gradient is not finite keeps every bit;
the driver logs the three scalars, run to run and across a resume; two ranks hold the same bits."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import clip_ref as CR
import momentum_ref as MR
from test_gpu_clip import bits, within_one_ulp
from test_gpu_dcnf_pairwise_train import batch_for, start_params
from test_gpu_momentum_train import (B, COARSE, FINE, MU, assert_states_equal, batch, params, reset_plugin, same, same_weights,  # noqa: F401
                                     state, train, unfused)
from test_gpu_valid_train import event_scalars, rows

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
INF = float('inf')


def read(group):
    from ann3depth_amd import ops
    return ops.clip_read(group.ctl)


def no_clip_attributes(net):
    names = list(vars(net)) + [n for g in net.groups.values() for n in vars(g)]
    return not any('clip' in n or n in ('ctl', 'ws') for n in names) and net.clip_norm is None


# ---------------------------------------------------------------------------------------------- None and inf
def test_without_the_argument_momentum_is_what_it_was(params, unfused):
    from ann3depth_amd import models
    net = models.MSDNReplica(B, params=params, optimizer='momentum', clip_norm=None)
    assert no_clip_attributes(net)
    for step in range(3):
        net.step(*batch(step))
        assert_states_equal(state(net), unfused[step + 1])


def test_without_the_argument_adam_is_what_it_was(params):
    from ann3depth_amd import models
    nets = [models.MSDNReplica(B, params=params, beta2=0.999, keep_dense_grads=False),
            models.MSDNReplica(B, params=params, beta2=0.999, keep_dense_grads=False, clip_norm=None)]
    for step in range(3):
        for net in nets:
            net.step(*batch(step))
    torch.cuda.synchronize()
    assert all(no_clip_attributes(net) and not net.keep_dense_grads for net in nets)
    for ga, gb in zip(nets[0].groups.values(), nets[1].groups.values()):
        for a, b in ((ga.var, gb.var), (ga.m, gb.m), (ga.v, gb.v)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), ga.name
        assert (float(ga.beta1_power), float(ga.beta2_power)) == (float(gb.beta1_power), float(gb.beta2_power))
        assert (float(ga.beta1_power) != float(np.float32(0.9))) == (ga.name in COARSE)


@pytest.fixture(scope='module')
def measured(params, unfused):
    """Three coarse steps under clip_norm=inf, asked for fused: the unfused, unclipped replica's bits; the norms of every step."""
    from ann3depth_amd import models
    net = models.MSDNReplica(B, params=params, optimizer='momentum', keep_dense_grads=False, clip_norm=INF)
    assert net.clip_norm == INF and net.keep_dense_grads and not net._fused_dense_momentum() and not net._fused_dense_adam()
    norms = []
    for step in range(3):
        net.step(*batch(step))
        assert_states_equal(state(net), unfused[step + 1])
        sts = {gn: read(net.groups[gn]) for gn in COARSE}
        for gn, st in sts.items():
            want = CR.clip(net.groups[gn].grad.cpu().numpy(), 1.0, INF)
            assert (st.skip, st.skipped) == (0, 0) and bits(st.scale) == bits(1.0) and within_one_ulp(st.norm, want.norm), gn
            assert 0 < st.norm < INF
        norms.append({gn: float(st.norm) for gn, st in sts.items()})
    assert all(not read(net.groups[gn]).sumsq for gn in FINE)                # never launched for the groups the phase leaves alone
    return norms


def test_inf_is_the_unfused_unclipped_step_in_the_coarse_phase(measured):
    assert len(measured) == 3


def test_inf_is_the_unclipped_step_in_the_fine_phase(params):
    from ann3depth_amd import models
    start = models.SAMPLES_COARSE // B
    nets = [models.MSDNReplica(B, params=params, optimizer='momentum', global_step=start, clip_norm=c) for c in (None, INF)]
    for net in nets:
        assert net.step(*batch(7))['phase'] == 2
    assert_states_equal(state(nets[0]), state(nets[1]))
    for gn in FINE:
        st = read(nets[1].groups[gn])
        assert bits(st.scale) == bits(1.0) and 0 < st.norm < INF and st.skip == 0
    rec = nets[1].summary_scalars({'coarse_loss': 0.0, 'fine_loss': 0.0, 'phase': 2})
    assert {k for k in rec if k.startswith('optimizers/') and k != 'optimizers/Phase'} == {
        f'optimizers/{tag}/{gn}' for tag in ('GradNorm', 'ClipScale', 'SkippedSteps') for gn in FINE}
    assert not any(k.startswith('optimizers/GradNorm') for k in nets[0].summary_scalars({'coarse_loss': 0.0, 'fine_loss': 0.0,
                                                                                          'phase': 2}))


# ---------------------------------------------------------------------------------------------- a bound below the norms
def test_clipped_momentum_steps_are_the_rule_at_each_groups_own_scale(params, measured):
    from ann3depth_amd import models
    C = 0.5 * min(measured[0].values())
    net = models.MSDNReplica(B, params=params, optimizer='momentum', clip_norm=C)
    before = state(net)
    for t in range(1, 4):
        assert net.step(*batch(t - 1))['phase'] == 1
        after = state(net)
        for gn, g in net.groups.items():
            if gn in FINE:
                assert same(after[gn][0], before[gn][0]) and same(after[gn][1], before[gn][1]), gn
                continue
            grad, st = g.grad.cpu().numpy(), read(g)
            want = CR.clip(grad, 1.0, C)
            assert st.skip == 0 and within_one_ulp(st.scale, want.scale) and within_one_ulp(st.norm, want.norm), (gn, st, want)
            assert t > 1 or st.scale < 1                                     # C is half the smallest norm of this very step
            var, accum = MR.step(before[gn][0], before[gn][1], grad, g.lr, g.momentum, st.scale)
            assert same(after[gn][1], accum) and same(after[gn][0], var) and not same(var, before[gn][0]), gn
            # after t clipped steps: each adds a gradient of norm <= C to mu times the last accumulator; two float32
            # roundings per element per step
            bound = float(np.float32(C)) * (1 - MU ** t) / (1 - MU) * (1 + t * 1e-6)
            assert np.linalg.norm(after[gn][1].astype(np.float64)) <= bound, (gn, t)
        before = after
    rec = net.summary_scalars({'coarse_loss': 0.0, 'fine_loss': 0.0, 'phase': 1})
    for gn in COARSE:
        st = read(net.groups[gn])
        assert rec[f'optimizers/GradNorm/{gn}'] == float(st.norm) and rec[f'optimizers/ClipScale/{gn}'] == float(st.scale)
        assert rec[f'optimizers/SkippedSteps/{gn}'] == 0
    assert not any(gn in k for k in rec for gn in FINE)


def test_a_clipped_adam_step_is_the_rule_at_each_groups_own_scale(params, measured):
    from ann3depth_amd import models, ops
    C = 0.5 * min(measured[0].values())
    net = models.MSDNReplica(B, params=params, beta2=0.999, keep_dense_grads=False, clip_norm=C)
    assert net.keep_dense_grads and not net._fused_dense_adam()
    old = {gn: [t.clone() for t in (g.var, g.m, g.v)] for gn, g in net.groups.items()}
    net.step(*batch(0))
    torch.cuda.synchronize()
    for gn, g in net.groups.items():
        if gn in COARSE:
            st = read(g)
            want = CR.clip(g.grad.cpu().numpy(), 1.0, C)
            assert st.skip == 0 and st.scale < 1 and within_one_ulp(st.scale, want.scale), (gn, st, want)
            ops.adam_apply_tf1(*old[gn], g.grad, g.lr, g.beta1, g.beta2, g.eps, g.beta1, g.beta2, float(st.scale))
            assert float(g.beta1_power) == float(np.float32(g.beta1) * np.float32(g.beta1))
        for got, want_t in zip((g.var, g.m, g.v), old[gn]):
            assert torch.equal(got.view(torch.int32), want_t.view(torch.int32)), gn


# ---------------------------------------------------------------------------------------------- a NaN in one image
def test_a_group_whose_gradient_is_not_finite_keeps_every_bit(params, measured):
    """A NaN in one image reaches conv2d_0's filter gradient whatever the activations do with it; whether it reaches the dense
    layers is the forward's business (a ReLU may stop it), so each group is held to its own gradient: not finite, nothing of it
    moves and skipped == 1; finite, it goes by the rule.  The next clean step moves everything; without the flag the same batch
    leaves NaN in the weights for good."""
    from ann3depth_amd import models
    C = 0.5 * min(measured[0].values())
    img, dep, keep = batch(0)
    img, dep = img.float() / 255, dep.float() / 255                          # stored as float32, where a NaN can be written
    bad = img.clone()
    bad[1, 20, 30, 1] = float('nan')
    net = models.MSDNReplica(B, params=params, optimizer='momentum', clip_norm=C)
    before = state(net)
    net.step(bad, dep, keep)
    after = state(net)
    skipped = {}
    for gn in COARSE:
        g, st = net.groups[gn], read(net.groups[gn])
        finite = bool(torch.isfinite(g.grad).all())
        skipped[gn] = st.skip
        assert st.skip == (0 if finite else 1) and st.skipped == st.skip, (gn, st)
        if st.skip:
            assert bits(st.scale) == bits(0.0)
            want = before[gn]
        else:
            want = MR.step(before[gn][0], before[gn][1], g.grad.cpu().numpy(), g.lr, g.momentum, st.scale)
        assert same(after[gn][0], want[0]) and same(after[gn][1], want[1]), gn
        assert np.isfinite(after[gn][0]).all() and np.isfinite(after[gn][1]).all(), gn
    assert skipped['CoarseConv'] == 1 and net.global_step == 1               # the step counts, the host does not know
    for gn in FINE:
        assert same(after[gn][0], before[gn][0])
    net.step(img, dep, keep)                                                 # the next clean step moves the weights
    moved = state(net)
    for gn in COARSE:
        st = read(net.groups[gn])
        assert (st.skip, st.skipped) == (0, skipped[gn]) and not same(moved[gn][0], after[gn][0]), gn
        assert np.isfinite(moved[gn][0]).all()
    plain = models.MSDNReplica(B, params=params, optimizer='momentum')
    plain.step(bad, dep, keep)
    assert np.isnan(state(plain)['CoarseConv'][0]).any()                     # what the flag buys


# ---------------------------------------------------------------------------------------------- DCNF
def test_dcnf_groups_descend_at_lr_times_scale_and_inf_is_todays_step():
    from ann3depth_amd import models, ops
    n, start = 2, start_params()
    plain = models.DCNFReplica(n, params=start, train_pairwise=True)
    assert plain.clip_norm is None and not hasattr(plain.pair_group, 'ctl') and not hasattr(plain.unary.group, 'ctl')
    img, dep = batch_for(plain, n, seed=21)
    measure = models.DCNFReplica(n, params=start, train_pairwise=True, clip_norm=INF)
    for rep in (plain, measure):
        rep.step(img, dep)
    torch.cuda.synchronize()
    norms = {}
    for gn in ('unary', 'pairwise'):
        assert torch.equal(plain.groups[gn].var.view(torch.int32), measure.groups[gn].var.view(torch.int32)), gn
        st = read(measure.groups[gn])
        assert bits(st.scale) == bits(1.0) and st.skip == 0 and 0 < st.norm < INF
        norms[gn] = float(st.norm)
    C = 0.5 * min(norms.values())
    rep = models.DCNFReplica(n, params=start, train_pairwise=True, clip_norm=C)
    old = {gn: g.var.clone() for gn, g in rep.groups.items()}
    rep.step(img, dep)
    torch.cuda.synchronize()
    for gn, g in rep.groups.items():
        st = read(g)
        want = CR.clip(g.grad.cpu().numpy(), 1.0, C)
        assert st.skip == 0 and st.scale < 1 and within_one_ulp(st.scale, want.scale), (gn, st, want)
        lr = float(np.float32(g.lr) * np.float32(st.scale))
        if gn == 'unary':
            ops.sgd_apply(old[gn], g.grad, lr)
        else:
            ops.sgd_apply_floor(old[gn], g.grad, lr, 0.0)
        assert torch.equal(g.var.view(torch.int32), old[gn].view(torch.int32)), gn
        assert not torch.equal(g.var, plain.groups[gn].var)
    rec = rep.summary_scalars({'mean_loss': 0.0})
    assert {k for k in rec if k.startswith('optimizers/')} == {f'optimizers/{tag}/{gn}' for tag in ('GradNorm', 'ClipScale', 'SkippedSteps')
                                                             for gn in ('unary', 'pairwise')}
    # without --train-pairwise the pairwise group is never applied: no control block, no scalars
    unary_only = models.DCNFReplica(n, params=start, clip_norm=C)
    assert not hasattr(unary_only.pair_group, 'ctl') and unary_only.pair_group.clip_norm is None
    unary_only.step(img, dep)
    assert {k for k in unary_only.summary_scalars({'mean_loss': 0.0}) if 'pairwise' in k} == set()
    with pytest.raises(ValueError, match='clip_norm'):
        models.DCNFReplica(n, params=start, clip_norm=0.0)


def test_bad_bounds_are_refused(params):
    from ann3depth_amd import models
    for bad in (0.0, -1.0, float('nan'), -INF):
        with pytest.raises(ValueError, match='clip_norm'):
            models.MSDNReplica(B, params=params, clip_norm=bad)
    assert models.msdn.clip_norm is None and models.dcnf.clip_norm is None


# ---------------------------------------------------------------------------------------------- the driver
def test_driver_logs_the_scalars_and_is_reproducible_and_resumable(tmp_path):
    from ann3depth_amd import models
    from test_gpu_valid_train import write_shard
    data, ck = str(tmp_path / 'data'), str(tmp_path / 'ckpt')
    write_shard(data, holes=False)
    C = 10.0
    tags = [f'optimizers/{tag}/{gn}' for tag in ('GradNorm', 'ClipScale', 'SkippedSteps') for gn in COARSE]
    try:
        a, sd = train(ck, data, 'a', 3, '--clip-norm', str(C))
        assert models.msdn.clip_norm == C
        recs = rows(ck, 'msdn_a')
        assert [r['global_step'] for r in recs] == [1, 2, 3]
        for r in recs:
            assert set(tags) <= set(r) and not any('Fine' in k for k in r)
            for gn in COARSE:
                norm, scale = r[f'optimizers/GradNorm/{gn}'], r[f'optimizers/ClipScale/{gn}']
                assert 0 < norm < INF and r[f'optimizers/SkippedSteps/{gn}'] == 0
                assert abs(scale - min(1.0, C / norm)) <= 2.0 ** -22 * scale      # two float32 roundings: the norm's and the scale's
        for tag in tags:
            assert event_scalars(ck, 'msdn_a', tag) == [float(np.float32(r[tag])) for r in recs], tag
        again, sd_again = train(ck, data, 'b', 3, '--clip-norm', str(C))
        logged = lambda run: [{k: v for k, v in r.items() if not k.endswith('/sec')} for r in rows(ck, run)]      # noqa: E731
        assert again == a and same_weights(sd_again, sd) and logged('msdn_b') == logged('msdn_a')      # the norms and scales too
        first, _ = train(ck, data, 'c', 2, '--clip-norm', str(C))
        resumed, sd_resumed = train(ck, data, 'c', 3, '--clip-norm', str(C))   # continues from the step-2 checkpoint
        assert first == {k: a[k] for k in (1, 2)} and resumed == a and same_weights(sd_resumed, sd)
        assert not any('clip' in k.lower() for k in sd)                      # nothing of it is in a checkpoint
    finally:
        models.msdn.clip_norm = None
        reset_plugin()


# ---------------------------------------------------------------------------------------------- two ranks
def test_two_ranks_clip_the_reduced_gradients_to_the_same_bits(tmp_path):
    """tests/clip_dp_worker.py: two ranks on the one GPU over gloo."""
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / 'ok.txt')
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), A3D_DIST_BACKEND='gloo')
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, 'clip_dp_worker.py'), out], env=env))
    for p in procs:
        assert p.wait(timeout=300) == 0
    assert open(out).read() == '1'
