"""The MSDN training step and the drivers under the scale-and-shift-invariant objective (MSDNReplica(objective='ssi'),
--loss ssi): 'silog' and 'berhu' replicas are what they were; under 'ssi' the four loss floats and the loss gradients are those
of tests/ssi_ref.py on the replica's own outputs and target, with and without holes, in both phases; the drivers, evaluate's
report, the refusals, and two data-parallel ranks against one replica on the concatenated batch."""
import json
import os
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import ssi_ref as R
from oracle import msdn as O
from test_gpu_berhu_train import NEW_TAGS as BERHU_TAGS
from test_gpu_berhu_train import restore_signals
from test_gpu_valid_train import event_scalars, fine_start, rows, stored_batch, write_shard

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
INF = float('inf')
B = 2
NEW_TAGS = ('loss/coarse_scale', 'loss/fine_scale', 'loss/coarse_shift', 'loss/fine_shift')


@pytest.fixture(scope='module')
def params():
    return O.init_params(3000)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('objective', ['silog', 'berhu'])
def test_the_other_objectives_are_what_they_were(params, objective):
    """No attribute, buffer, output or summary key of a 'silog' or 'berhu' replica knows of ssi."""
    from ann3depth_amd import models, ops
    img, dep, keep = stored_batch(1, holes=True)
    net = models.MSDNReplica(B, params=params, beta2=0.999, valid_range=(0, INF), objective=objective)
    assert not any('ssi' in name for name in vars(net)) and net.objective == objective
    assert ('objective' in vars(net)) == (objective == 'berhu') and ('berhu_fraction' in vars(net)) == (objective == 'berhu')
    want_ws = ops.berhu_ws if objective == 'berhu' else ops.silog_masked_ws
    assert net.ws_c.numel() == want_ws(B, 'cpu').numel() and net.loss_out_c.numel() == (4 if objective == 'berhu' else 2)
    out = net.step(dev(img), dev(dep), dev(keep))
    torch.cuda.synchronize()
    assert sorted(out) == ['coarse_loss', 'fine_loss', 'phase'] and np.isfinite(float(out['coarse_loss']))
    keys = {'loss/coarse_loss', 'loss/fine_loss', 'optimizers/Phase', 'valid_fraction'}
    assert set(net.summary_scalars(out)) == keys | (set(BERHU_TAGS) if objective == 'berhu' else set())
    assert models.msdn_loss_launches(objective, 0.2, 0.0, True).name == ('berhu' if objective == 'berhu' else None)
    assert models.msdn_loss_launches('ssi', 0.2, 0.0, True)[:2] == (4, 'ssi')


@pytest.mark.parametrize('holes', [False, True])
def test_ssi_step_is_the_reference(params, holes):
    from ann3depth_amd import models, ops
    img, dep, keep = stored_batch(2, holes=holes)
    masked = int(holes)
    net = models.MSDNReplica(B, params=params, beta2=0.999, valid_range=(0.0, 0.99) if holes else None, objective='ssi')
    assert net.ws_c.numel() == ops.ssi_ws(B, 'cpu').numel() and net.loss_out_c.numel() == 4 and net.objective == 'ssi'
    assert 'berhu_fraction' not in vars(net) and net.loss_ssi_c is net.loss_out_c
    for start in (0, fine_start(models)):
        net.global_step = start
        out = net.step(dev(img), dev(dep), dev(keep))
        torch.cuda.synchronize()
        t = net.t.cpu().numpy().reshape(B, -1)
        hole = ~np.isfinite(t)
        assert (0.02 < hole.mean() < 0.5) if holes else not hole.any()
        scalars = net.summary_scalars(out)
        for which, quad, ws in (('coarse', net.loss_ssi_c, net.ws_c), ('fine', net.loss_ssi_f, net.ws_f)):
            o = getattr(net, which).cpu().numpy().reshape(B, -1)
            ref, b_loss, b_s, b_t, b_grad = R.bound(o, t, masked)
            l64, g64, s64, t64, flag64, n64 = ref
            got = quad.cpu().numpy()
            e_loss, e_s, e_t, _ = R.errors(got, g64, ref)
            print(f'{which} start {start} holes {holes}: loss {e_loss:.2e} (bound {b_loss:.2e}), scale {e_s:.2e} ({b_s:.2e}), '
                  f'shift {e_t:.2e} ({b_t:.2e}); loss {l64[0]:.6g} scale {l64[2]:.6g} shift {l64[3]:.6g}')
            assert np.isfinite(got).all() and (flag64 == R.FITTED).all() and l64[0] > 0
            assert e_loss <= b_loss and e_s <= b_s and e_t <= b_t
            assert got[1] == np.float32((~hole).mean())
            per = ws.cpu().numpy()[2:2 + 4 * B].reshape(B, 4)
            np.testing.assert_array_equal(per[:, 2], (~hole).sum(axis=1).astype(np.float32))
            assert (per[:, 3] == 0).all()
            # the summary scalars are the buffers' values
            assert float(out[which + '_loss']) == got[0] and scalars[f'loss/{which}_loss'] == float(got[0])
            assert scalars[f'loss/{which}_scale'] == float(got[2]) and scalars[f'loss/{which}_shift'] == float(got[3])
            if which != ('coarse' if start == 0 else 'fine'):
                continue
            g = (net.dz1 if start == 0 else net.dfine).cpu().numpy().reshape(B, -1)
            e_grad = R.grad_err(g, g64)
            print(f'  d{which}: {e_grad:.2e} (bound {b_grad:.2e})')
            assert b_grad > 0 and e_grad <= b_grad and np.isfinite(g).all()
            assert (g[hole].view(np.uint32) == 0).all() and (g[~hole] != 0).mean() > 0.99
            # the pull does not move the output's mean and does not scale it: the two directions the fit removes
            for i in range(B):
                gi, oi = g[i][~hole[i]].astype(np.float64), o[i][~hole[i]].astype(np.float64)
                assert abs(gi.sum()) <= 1e-4 * np.abs(gi).sum() and abs((gi * oi).sum()) <= 1e-4 * np.abs(gi * oi).sum()
        assert ('valid_fraction' in scalars) == holes and set(NEW_TAGS) <= set(scalars) and not set(BERHU_TAGS) & set(scalars)
    for gname in net.groups:
        assert bool(torch.isfinite(net.groups[gname].var).all()), gname


def test_bf16_storage_takes_the_gradient_as_bf16_rows(params):
    from ann3depth_amd import models
    img, dep, keep = stored_batch(5, holes=True)
    net = models.MSDNReplica(B, params=params, beta2=0.999, precision='bf16s', valid_range=(0, INF), objective='ssi')
    out = net.step(dev(img), dev(dep), dev(keep))
    torch.cuda.synchronize()
    assert np.isfinite(float(out['coarse_loss'])) and np.isfinite(float(out['fine_loss'])) and float(net.loss_ssi_c[2]) != 0
    dz1, dz16 = net.dz1.cpu(), net.dz1_16.float().cpu()
    assert torch.equal(dz16[:, :4070], dz1.to(torch.bfloat16).float()) and bool((dz16[:, 4070:] == 0).all())
    hole = ~np.isfinite(net.t.cpu().numpy().reshape(B, -1))
    assert hole.any() and bool((dz1.numpy()[hole] == 0).all()) and bool((dz1 != 0).any())


def test_ssi_step_under_augmentation(params):
    """A warp table of --augment eigen beside holes: the loss launches see the warped target, nothing else changes."""
    from ann3depth_amd import augment as A
    from ann3depth_amd import models
    img, dep, keep = stored_batch(3, holes=True)
    net = models.MSDNReplica(B, params=params, beta2=0.999, valid_range=(0, INF), objective='ssi')
    out = net.step(dev(img), dev(dep), dev(keep), warp=dev(A.table(A.Eigen2014(), 3000, 0, 1, B, 48, 64)))
    torch.cuda.synchronize()
    o, t = net.coarse.cpu().numpy().reshape(B, -1), net.t.cpu().numpy().reshape(B, -1)
    ref, b_loss, b_s, b_t, b_grad = R.bound(o, t, 1)
    e_loss, e_s, e_t, e_grad = R.errors(net.loss_ssi_c.cpu().numpy(), net.dz1.cpu().numpy().reshape(B, -1), ref)
    print(f'ssi under a warp table: loss {e_loss:.2e} ({b_loss:.2e}), gradient {e_grad:.2e} ({b_grad:.2e})')
    assert 0 < (~np.isfinite(t)).mean() < 0.5 and np.isfinite(float(out['coarse_loss'])) and (ref[4] == R.FITTED).all()
    assert e_loss <= b_loss and e_s <= b_s and e_t <= b_t and e_grad <= b_grad


def test_bad_objectives_and_combinations_are_refused(params):
    from ann3depth_amd import models
    with pytest.raises(ValueError, match="'silog', 'berhu' or 'ssi'"):
        models.MSDNReplica(B, params=params, objective='l2')
    with pytest.raises(ValueError, match="'ssi' with grad_weight"):
        models.MSDNReplica(B, params=params, objective='ssi', grad_weight=0.5)
    with pytest.raises(ValueError, match='grad_weight'):
        models.MSDNReplica(B, params=params, objective='ssi', grad_weight=-1.0)
    assert models.msdn.objective == 'silog'


# ---------------------------------------------------------------------------------------------- the drivers
def losses(ck, run):
    return {r['global_step']: (r['loss/coarse_loss'], r['loss/fine_loss']) + tuple(r.get(tag) for tag in NEW_TAGS)
            for r in rows(ck, run)}


def train(ck, data, run_id, steps, *flags):
    from ann3depth_amd import ann3depth
    argv = ['--model', 'msdn', '--batchsize', '4', '--ckptdir', ck, '--datadir', data, '--sumfreq', '1', '--trace-every', '0',
            '--beta2', '0.999', '--min-depth', '0', '--id', run_id, '--steps', str(steps), *flags, 'nyu']
    assert ann3depth.main(argv) == 0
    return losses(ck, 'msdn_' + run_id)


def reset_plugin():
    from ann3depth_amd import models
    models.msdn.valid_range = None
    models.msdn.objective = 'silog'
    models.msdn.berhu_fraction = 0.2
    models.msdn.beta2 = 1.0                      # --beta2 stays on the plugin; the tests after this one train without the flag
    restore_signals()


@pytest.fixture(scope='module')
def trained(tmp_path_factory):
    """A shard with holes (the same records as its test split) and run `a`: four steps under --loss ssi, shared by the two
    driver tests below."""
    from ann3depth_amd import models
    root = tmp_path_factory.mktemp('ssi')
    data, ck = str(root / 'holed'), str(root / 'ckpt')
    write_shard(data, holes=True)
    shutil.copy(os.path.join(data, 'nyu', 'train.tfrecords'), os.path.join(data, 'nyu', 'test.tfrecords'))
    try:
        a = train(ck, data, 'a', 4, '--loss', 'ssi')
        assert models.msdn.objective == 'ssi'
    finally:
        reset_plugin()
    return ck, data, a


def test_driver_under_ssi_is_reproducible_and_resumable(trained):
    from ann3depth_amd import models
    ck, data, a = trained
    try:
        assert sorted(a) == [1, 2, 3, 4]
        assert all(v is not None and np.isfinite(v) for six in a.values() for v in six) and len(set(a.values())) == 4
        first = train(ck, data, 'c', 2, '--loss', 'ssi')
        resumed = train(ck, data, 'c', 4, '--loss', 'ssi')                 # continues from the step-2 checkpoint
        assert first == {k: a[k] for k in (1, 2)} and resumed == a        # a second run, and a resumed one: the same values
        for col, tag in enumerate(NEW_TAGS, start=2):
            logged = event_scalars(ck, 'msdn_a', tag)
            assert logged == [float(np.float32(a[k][col])) for k in sorted(a)] and all(v != 0 for v in logged)
        assert len(event_scalars(ck, 'msdn_a', 'valid_fraction')) == 4     # stays as it is
        # the four new tags and no others
        known = {'global_step', 'loss/coarse_loss', 'loss/fine_loss', 'valid_fraction'}
        without = train(ck, data, 'f', 1)
        plain_keys = set().union(*(set(r) for r in rows(ck, 'msdn_f')))
        ssi_keys = set().union(*(set(r) for r in rows(ck, 'msdn_a')))
        assert known <= plain_keys and ssi_keys - plain_keys == set(NEW_TAGS) and plain_keys <= ssi_keys
        # the default: the scale-invariant log loss, and no new tag
        assert models.msdn.objective == 'silog' and all(v is None for v in without[1][2:]) and without[1][:2] != a[1][:2]
        for tag in NEW_TAGS:
            assert event_scalars(ck, 'msdn_f', tag) == []
    finally:
        reset_plugin()


def test_evaluate_reports_ssi_only_when_asked(trained, capsys):
    """The checkpoint of the ssi run restores wherever an MSDN checkpoint does; `ssi` appears beside `silog` with the flag."""
    from ann3depth_amd import evaluate
    ck, data, _ = trained
    base = ['--model', 'msdn', '--batchsize', '4', '--ckptdir', ck, '--datadir', data, '--id', 'a']
    capsys.readouterr()
    assert evaluate.main(base + ['nyu']) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert evaluate.main(base + ['--loss', 'ssi', 'nyu']) == 0
    got = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert plain['global_step'] == 4 and set(got) - set(plain) == {'loss'} and got['loss'] == 'ssi'
    for name in ('coarse', 'fine'):
        assert 'ssi' not in plain[name] and set(got[name]) - set(plain[name]) == {'ssi'}
        assert np.isfinite(got[name]['ssi']) and got[name]['ssi'] > 0
        for k in plain[name]:
            assert json.dumps(got[name][k]) == json.dumps(plain[name][k]), (name, k)
    # refused before any GPU work
    assert evaluate.main(['--model', 'dcnf', '--ckptdir', ck, '--datadir', data, '--loss', 'ssi', 'nyu']) == 2
    assert evaluate.main(base + ['--loss', 'ssi', '--berhu-fraction', '0.5', 'nyu']) == 2


def test_cli_refusals_come_before_anything_is_set_up(tmp_path):
    from ann3depth_amd import ann3depth
    try:
        common = ['--ckptdir', str(tmp_path), '--datadir', str(tmp_path)]
        assert ann3depth.main(['--model', 'dcnf', *common, '--loss', 'ssi', 'nyu']) == 2
        assert ann3depth.main(['--model', 'msdn', *common, '--loss', 'ssi', '--loss-gradient', '0.5', 'nyu']) == 2
        assert ann3depth.main(['--model', 'msdn', *common, '--loss', 'ssi', '--loss-gradient', '0', 'nyu']) == 2
        assert ann3depth.main(['--model', 'msdn', *common, '--loss', 'ssi', '--berhu-fraction', '0.5', 'nyu']) == 2
        assert not os.listdir(tmp_path)                                    # refused before anything was set up
    finally:
        restore_signals()


def test_two_ranks_equal_one_rank_on_the_concatenated_batch(tmp_path):
    """tests/ssi_dp_worker.py: two ranks on the one GPU over gloo."""
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / 'ok.txt')
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), A3D_DIST_BACKEND='gloo')
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, 'ssi_dp_worker.py'), out], env=env))
    for p in procs:
        assert p.wait(timeout=300) == 0
    assert open(out).read() == '1'
