"""The MSDN training step and the drivers under SGD with momentum (MSDNReplica(optimizer='momentum'), --optimizer momentum):
every variable and accumulator after a step is tests/momentum_ref.py applied on the host to the values before it and to the
replica's own gradients, bit for bit, in both phases; the fused dense path (keep_dense_grads=False) leaves the same bits; an
Adam replica is what it was; the refusals, the checkpoints (which restore only under the optimizer that wrote them), the
training driver, evaluate and predict, and two data-parallel ranks."""
import os
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import momentum_ref as MR
from oracle import msdn as O
from test_gpu_berhu_train import restore_signals
from test_gpu_valid_train import rows, stored_batch, write_shard

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
B = 4
MU = 0.9
COARSE, FINE = ('CoarseConv', 'CoarseDense'), ('FineA', 'FineB')


@pytest.fixture(scope='module')
def params():
    return O.init_params(3000)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def batch(seed):
    """Four records: two stored batches of two."""
    return [dev(np.concatenate(pair)) for pair in zip(stored_batch(seed, holes=False), stored_batch(seed + 100, holes=False))]


def state(net):
    """{group: (var, accumulator)} on the host."""
    net.settle()
    torch.cuda.synchronize()
    return {gn: (g.var.cpu().numpy(), g.m.cpu().numpy()) for gn, g in net.groups.items()}


def same(a, b):
    a, b = (np.ascontiguousarray(x, np.float32) for x in (a, b))
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def assert_states_equal(a, b):
    for gn in a:
        assert same(a[gn][0], b[gn][0]), gn + ' var'
        assert same(a[gn][1], b[gn][1]), gn + ' accumulator'


def assert_step_is_the_rule(net, before, moved, scale=1.0):
    """Every group in `moved` went by the rule on the replica's own gradient; the others kept every bit."""
    after = state(net)
    for gn, g in net.groups.items():
        if gn in moved:
            var, accum = MR.step(before[gn][0], before[gn][1], g.grad.cpu().numpy(), g.lr, g.momentum, scale)
            assert np.any(accum != before[gn][1]) and not same(var, before[gn][0]), gn
        else:
            var, accum = before[gn]
        assert same(after[gn][1], accum), gn + ' accumulator'
        assert same(after[gn][0], var), gn + ' var'
    return after


@pytest.fixture(scope='module')
def unfused(params):
    """Three coarse-phase steps with the dense gradients kept, each held to the rule; the state after every step, for the fused
    path to equal."""
    from ann3depth_amd import models
    net = models.MSDNReplica(B, params=params, optimizer='momentum', keep_dense_grads=True)
    assert net.optimizer == 'momentum' and net.momentum == MU and all(g.v is None for g in net.groups.values())
    assert all(g.optimizer == 'momentum' and not g.frozen() for g in net.groups.values()) and not net._m_sharded
    assert [g.lr for g in net.groups.values()] == [0.001, 0.1, 0.001, 0.01]
    states = [state(net)]
    losses = []
    for step in range(3):
        out = net.step(*batch(step))
        assert out['phase'] == 1
        states.append(assert_step_is_the_rule(net, states[-1], COARSE))
        losses.append(float(out['coarse_loss']))
    assert all(np.isfinite(l) for l in losses) and net.global_step == 3
    return states


def test_three_coarse_steps_are_the_rule_on_the_replicas_own_gradients(unfused):
    first, last = unfused[0], unfused[-1]
    for gn in COARSE:
        assert not first[gn][1].any() and last[gn][1].any() and (first[gn][0] != last[gn][0]).mean() > 0.1      # (dropout and dead units leave many gradients at zero)
    for gn in FINE:
        assert same(first[gn][0], last[gn][0]) and not last[gn][1].any()


def test_the_fused_dense_path_leaves_the_same_bits(params, unfused, monkeypatch):
    from ann3depth_amd import models, ops
    calls = []
    real = ops.dense_bwd_filter_momentum

    def spy(x, dz, *rest):
        calls.append((tuple(x.shape), tuple(dz.shape)))
        return real(x, dz, *rest)
    monkeypatch.setattr(ops, 'dense_bwd_filter_momentum', spy)
    net = models.MSDNReplica(B, params=params, optimizer='momentum', keep_dense_grads=False)
    assert net._fused_dense_momentum() and not net._fused_dense_adam()
    for step in range(3):
        net.step(*batch(step))
        assert_states_equal(state(net), unfused[step + 1])
    assert len(calls) == 6 and sorted(calls[:2]) == sorted(calls[2:4]) == sorted(calls[4:]) == [((B, 4096), (B, 4070)), ((B, 12288), (B, 4096))]
    assert not net.grad('coarse/dense/dense_0/kernel').any()                  # the dense gradient was never written


def test_a_fine_phase_step_moves_the_fine_groups_only(params):
    from ann3depth_amd import models
    net = models.MSDNReplica(B, params=params, optimizer='momentum', global_step=models.SAMPLES_COARSE // B)
    before = state(net)
    out = net.step(*batch(7))
    assert out['phase'] == 2
    assert_step_is_the_rule(net, before, FINE)


def test_lr_scale_multiplies_the_rates_and_nothing_else(params):
    from ann3depth_amd import models
    nets = [models.MSDNReplica(B, params=params, optimizer='momentum', lr_scale=s) for s in (1.0, 0.5)]
    assert 'lr_scale' not in vars(nets[0]) and nets[1].lr_scale == 0.5
    assert [g.lr for g in nets[1].groups.values()] == [0.0005, 0.05, 0.0005, 0.005]
    before = state(nets[0])
    for net in nets:
        net.step(*batch(3))
    whole, half = assert_step_is_the_rule(nets[0], before, COARSE), assert_step_is_the_rule(nets[1], before, COARSE)
    for gn in COARSE:
        assert same(whole[gn][1], half[gn][1])                             # the accumulator does not know the rate
        # half the rate is half the product lr accum, exactly (a power of two; nothing here is denormal)
        lr = np.float32(nets[0].groups[gn].lr)
        assert same(half[gn][0], before[gn][0] - (lr * whole[gn][1]) * np.float32(0.5))
    adam = models.MSDNReplica(B, params=params, beta2=0.999, lr_scale=0.5)
    assert [g.lr for g in adam.groups.values()] == [0.0005, 0.05, 0.0005, 0.005] and adam.optimizer == 'adam'


def test_bf16_storage_under_momentum_refreshes_the_weight_copies(params):
    from ann3depth_amd import models, ops
    net = models.MSDNReplica(B, params=params, optimizer='momentum', precision='bf16s', keep_dense_grads=False)
    before = state(net)
    losses = [net.step(*batch(step)) for step in range(2)]
    after = state(net)
    assert all(np.isfinite(float(o['coarse_loss'])) and np.isfinite(float(o['fine_loss'])) for o in losses)
    assert not same(after['CoarseDense'][0], before['CoarseDense'][0]) and net.wcopy
    for name, copy in net.wcopy.items():
        want = ops.cast_bf16(net.var(name + '/kernel'), torch.empty_like(copy))
        assert torch.equal(copy.view(torch.int16), want.view(torch.int16)), name


def test_adam_is_what_it_was(params):
    from ann3depth_amd import models
    nets = [models.MSDNReplica(B, params=params, beta2=0.999), models.MSDNReplica(B, params=params, beta2=0.999, optimizer='adam',
                                                                                   lr_scale=1.0)]
    for step in range(2):
        for net in nets:
            net.step(*batch(step))
    torch.cuda.synchronize()
    for net in nets:
        names = list(vars(net)) + [n for g in net.groups.values() for n in vars(g)] + list(net.state_dict())
        assert not any('momentum' in n or n in ('optimizer', 'lr_scale') for n in names)
        assert net.optimizer == 'adam' and all(g.v is not None and g.optimizer == 'adam' for g in net.groups.values())
    for ga, gb in zip(nets[0].groups.values(), nets[1].groups.values()):
        for a, b in ((ga.var, gb.var), (ga.m, gb.m), (ga.v, gb.v)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), ga.name
        assert (ga.lr, float(ga.beta1_power), float(ga.beta2_power)) == (gb.lr, float(gb.beta1_power), float(gb.beta2_power))
    assert list(nets[0].state_dict()) == list(nets[1].state_dict())


def test_bad_optimizers_and_combinations_are_refused(params):
    from ann3depth_amd import models
    with pytest.raises(ValueError, match="'adam' or 'momentum'"):
        models.MSDNReplica(B, params=params, optimizer='sgd')
    for momentum in (-0.1, 1.0, float('nan')):
        with pytest.raises(ValueError, match=r'momentum .*\[0, 1\)'):
            models.MSDNReplica(B, params=params, optimizer='momentum', momentum=momentum)
    for lr_scale in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='lr_scale'):
            models.MSDNReplica(B, params=params, lr_scale=lr_scale)
    with pytest.raises(ValueError, match='beta2'):
        models.MSDNReplica(B, params=params, optimizer='momentum', beta2=0.999)
    assert models.msdn.optimizer == 'adam'


def test_cli_refusals_come_before_anything_is_set_up(tmp_path):
    from ann3depth_amd import ann3depth
    try:
        common = ['--ckptdir', str(tmp_path), '--datadir', str(tmp_path)]
        for flags in (['--optimizer', 'momentum'], ['--momentum', '0.5'], ['--lr-scale', '2']):
            assert ann3depth.main(['--model', 'dcnf', *common, *flags, 'nyu']) == 2
        msdn = ['--model', 'msdn', *common]
        assert ann3depth.main([*msdn, '--optimizer', 'momentum', '--beta2', '0.999', 'nyu']) == 2
        assert ann3depth.main([*msdn, '--momentum', '0.5', 'nyu']) == 2
        assert ann3depth.main([*msdn, '--optimizer', 'adam', '--momentum', '0.5', 'nyu']) == 2
        for bad in ('1', '-0.5', 'nan'):
            assert ann3depth.main([*msdn, '--optimizer', 'momentum', '--momentum', bad, 'nyu']) == 2
        for bad in ('0', '-1', 'inf', 'nan'):
            assert ann3depth.main([*msdn, '--lr-scale', bad, 'nyu']) == 2
            assert ann3depth.main([*msdn, '--optimizer', 'momentum', '--lr-scale', bad, 'nyu']) == 2
        assert not os.listdir(tmp_path)                                    # refused before anything was set up
    finally:
        restore_signals()


# ---------------------------------------------------------------------------------------------- checkpoints
def test_state_dict_round_trip_and_the_other_optimizers_checkpoint(params, unfused):
    from ann3depth_amd import models
    net = models.MSDNReplica(B, params=params, optimizer='momentum')
    for step in range(2):
        net.step(*batch(step))
    assert_states_equal(state(net), unfused[2])
    sd = net.state_dict()
    slots = {n + '/' + net.group_of[n] for n in net.shapes}
    assert set(sd) == set(net.shapes) | slots | {'global_step', 'optimizer'} and sd['optimizer'] == 'momentum'
    assert not any(k.endswith('_1') or 'power' in k for k in sd) and models.checkpoint_optimizer(sd) == 'momentum'
    tf = net.tf_variables()
    assert set(tf) == set(sd) - {'optimizer'} and models.checkpoint_optimizer(tf) == 'momentum'
    saved = {k: v.detach().cpu().clone() if torch.is_tensor(v) else v for k, v in sd.items()}
    fresh = models.MSDNReplica(B, optimizer='momentum', seed=1)
    fresh.load_state_dict(saved)
    assert fresh.global_step == 2
    assert_states_equal(state(fresh), unfused[2])
    fresh.step(*batch(2))                                                  # ... and continues bit-identically
    assert_states_equal(state(fresh), unfused[3])
    other = models.MSDNReplica(B, params=params)
    with pytest.raises(ValueError, match=r"'momentum'.*'adam'.*--optimizer momentum"):
        other.load_state_dict(saved)
    with pytest.raises(ValueError, match=r"'momentum'.*'adam'.*--optimizer momentum"):
        other.load_tf_variables(tf)
    adam_state = {k: v.detach().cpu().clone() for k, v in other.state_dict().items()}
    assert 'optimizer' not in adam_state and models.checkpoint_optimizer(adam_state) == 'adam'
    with pytest.raises(ValueError, match=r"'adam'.*'momentum'.*--optimizer adam"):
        net.load_state_dict(adam_state)
    assert_states_equal(state(net), unfused[2])                            # a refused restore touched nothing


# ---------------------------------------------------------------------------------------------- the drivers
def weights(path):
    sd = torch.load(path, map_location='cpu')
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in sd.items()}


def train(ck, data, run_id, steps, *flags):
    from ann3depth_amd import ann3depth
    argv = ['--model', 'msdn', '--batchsize', '4', '--ckptdir', ck, '--datadir', data, '--sumfreq', '1', '--trace-every', '0',
            '--optimizer', 'momentum', '--id', run_id, '--steps', str(steps), *flags, 'nyu']
    assert ann3depth.main(argv) == 0
    got = {r['global_step']: (r['loss/coarse_loss'], r['loss/fine_loss']) for r in rows(ck, 'msdn_' + run_id)}
    return got, weights(os.path.join(ck, 'msdn_' + run_id, f'model.ckpt-{steps}.pt'))


def reset_plugin():
    from ann3depth_amd import models
    models.msdn.optimizer, models.msdn.momentum, models.msdn.lr_scale = 'adam', 0.9, 1.0
    restore_signals()


def same_weights(a, b):
    assert sorted(a) == sorted(b)
    return all(a[k] == b[k] if isinstance(a[k], str) else same(a[k].astype(np.float32), b[k].astype(np.float32)) for k in a)


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """A shard (the same records as its test split) and run `a`: four steps under --optimizer momentum with TF bundles beside."""
    from ann3depth_amd import models
    root = tmp_path_factory.mktemp('momentum')
    data, ck = str(root / 'data'), str(root / 'ckpt')
    write_shard(data, holes=False)
    shutil.copy(os.path.join(data, 'nyu', 'train.tfrecords'), os.path.join(data, 'nyu', 'test.tfrecords'))
    try:
        losses, sd = train(ck, data, 'a', 4, '--tf-checkpoints')
        assert models.msdn.optimizer == 'momentum' and models.msdn.momentum == 0.9 and models.msdn.lr_scale == 1.0
    finally:
        reset_plugin()
    return ck, data, losses, sd


def test_driver_under_momentum_is_reproducible_and_resumable(trained, params):
    from ann3depth_amd import models
    ck, data, a, sd = trained
    try:
        assert sorted(a) == [1, 2, 3, 4] and all(np.isfinite(v) for pair in a.values() for v in pair)
        assert len({pair[0] for pair in a.values()}) == 4                  # the weights moved: every step's loss is another
        assert sd['optimizer'] == 'momentum' and models.checkpoint_optimizer(sd) == 'momentum' and int(sd['global_step']) == 4
        name = 'coarse/dense/dense_1/kernel'
        assert sd[name + '/CoarseDense'].any() and name + '/CoarseDense_1' not in sd
        again, sd_again = train(ck, data, 'b', 4)
        assert again == a and same_weights(sd_again, sd)                   # run to run
        first, _ = train(ck, data, 'c', 2)
        resumed, sd_resumed = train(ck, data, 'c', 4)                      # continues from the step-2 checkpoint
        assert first == {k: a[k] for k in (1, 2)} and resumed == a and same_weights(sd_resumed, sd)
        scaled, sd_scaled = train(ck, data, 'd', 1, '--lr-scale', '0.5', '--momentum', '0.5')
        assert models.msdn.lr_scale == 0.5 and models.msdn.momentum == 0.5 and sd_scaled['optimizer'] == 'momentum'      # the flags reach the plugin
    finally:
        reset_plugin()


def test_the_bundle_reads_as_momentum_and_restores(trained):
    from ann3depth_amd import ann3depth, models
    ck, data, _, sd = trained
    state, bundle = ann3depth.read_checkpoint(os.path.join(ck, 'msdn_a', 'model.ckpt-4'), 'cpu')
    assert bundle and 'optimizer' not in state and models.checkpoint_optimizer(state) == 'momentum'
    net = models.MSDNReplica(B, optimizer='momentum', seed=2)
    ann3depth.load_checkpoint(net, state, bundle)
    assert net.global_step == 4
    for n in net.shapes:
        assert same(net.var(n).cpu().numpy(), sd[n]) and same(net.slot(n, 'm').cpu().numpy(), sd[n + '/' + net.group_of[n]]), n
    with pytest.raises(ValueError, match='--optimizer momentum'):
        ann3depth.load_checkpoint(models.MSDNReplica(B, seed=2), state, bundle)


def test_evaluate_and_predict_restore_the_run_with_no_new_flag(trained, tmp_path, capsys):
    from ann3depth_amd import evaluate, png, predict
    ck, data, _, _ = trained
    try:
        assert evaluate.main(['--model', 'msdn', '--batchsize', '4', '--ckptdir', ck, '--datadir', data, '--id', 'a', 'nyu']) == 0
        img = str(tmp_path / 'img.png')
        png.imsave(img, np.random.default_rng(5).integers(0, 256, (48, 64, 3)).astype(np.uint8))
        ckpt = os.path.join(ck, 'msdn_a', 'model.ckpt-4.pt')
        assert predict.main(['--model', 'msdn', '--checkpoint', ckpt, '--batchsize', '2', '--out', str(tmp_path / 'out'), img]) == 0
        assert np.isfinite(np.load(str(tmp_path / 'out' / 'img-depth.npy'))).all()
    finally:
        restore_signals()
        capsys.readouterr()


def test_two_ranks_apply_the_rule_to_the_reduced_gradients(tmp_path):
    """tests/momentum_dp_worker.py: two ranks on the one GPU over gloo."""
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / 'ok.txt')
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), A3D_DIST_BACKEND='gloo')
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, 'momentum_dp_worker.py'), out], env=env))
    for p in procs:
        assert p.wait(timeout=300) == 0
    assert open(out).read() == '1'
