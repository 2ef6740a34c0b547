"""The MSDN training step and the drivers under the reverse Huber objective (MSDNReplica(objective='berhu'), --loss berhu):
objective='silog' is today's step bit for bit; under 'berhu' the four loss floats and the loss gradients are those of
tests/berhu_ref.py on the replica's own outputs and target, with and without holes, and outputs at or below zero are pulled
on, which the scale-invariant log loss cannot do."""
import json
import os
import shutil
import signal

import numpy as np
import pytest
import torch

import berhu_ref as R
from oracle import msdn as O
from test_gpu_valid_train import event_scalars, fine_start, rows, stored_batch, write_shard

pytestmark = pytest.mark.gpu

INF = float('inf')
B = 2
FRACTION = 0.2
NEW_TAGS = ('loss/coarse_threshold', 'loss/fine_threshold', 'loss/coarse_quadratic', 'loss/fine_quadratic')


@pytest.fixture(scope='module')
def params():
    return O.init_params(3000)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('valid_range', [None, (0, INF)])
def test_objective_silog_is_the_plain_step(params, valid_range):
    from ann3depth_amd import models
    img, dep, keep = stored_batch(1, holes=valid_range is not None)
    nets = [models.MSDNReplica(B, params=params, beta2=0.999, valid_range=valid_range),
            models.MSDNReplica(B, params=params, beta2=0.999, valid_range=valid_range, objective='silog')]
    assert sorted(vars(nets[0])) == sorted(vars(nets[1]))                                 # not one attribute or buffer more
    assert not any('berhu' in name for name in vars(nets[1])) and 'objective' not in vars(nets[1]) and nets[1].objective == 'silog'
    assert nets[0].ws_c.numel() == nets[1].ws_c.numel() and nets[0].loss_out_c.numel() == nets[1].loss_out_c.numel()
    for start in (0, fine_start(models)):
        outs = []
        for net in nets:
            net.global_step = start
            outs.append(net.step(dev(img), dev(dep), dev(keep)))
        torch.cuda.synchronize()
        assert outs[0]['phase'] == outs[1]['phase'] == (1 if start == 0 else 2)
        for k in ('coarse_loss', 'fine_loss'):
            assert torch.equal(outs[0][k], outs[1][k]) and np.isfinite(float(outs[0][k])), k
        for name in ('x', 'coarse', 'fine', 'dz1' if start == 0 else 'dfine'):
            assert torch.equal(getattr(nets[0], name), getattr(nets[1], name)), name
        for gname in nets[0].groups:
            ga, gb = nets[0].groups[gname], nets[1].groups[gname]
            for buf in ('grad', 'var', 'm', 'v'):
                assert torch.equal(getattr(ga, buf), getattr(gb, buf)), f'{gname}.{buf}'
        assert sorted(nets[1].summary_scalars(outs[1])) == sorted(nets[0].summary_scalars(outs[0]))      # no key is added
    assert float(nets[0].groups['CoarseDense'].m.abs().sum()) > 0 and float(nets[0].groups['FineA'].m.abs().sum()) > 0


def rel_l2(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(x - ref) / max(np.linalg.norm(ref), 1e-300))


@pytest.mark.parametrize('holes', [False, True])
def test_berhu_step_is_the_reference(params, holes):
    from ann3depth_amd import models, ops
    img, dep, keep = stored_batch(2, holes=holes)
    masked = int(holes)
    net = models.MSDNReplica(B, params=params, beta2=0.999, valid_range=(0.0, 0.99) if holes else None, objective='berhu',
                             berhu_fraction=FRACTION)
    assert net.ws_c.numel() == ops.berhu_ws(B, 'cpu').numel() and net.loss_out_c.numel() == 4
    for start in (0, fine_start(models)):
        net.global_step = start
        out = net.step(dev(img), dev(dep), dev(keep))
        torch.cuda.synchronize()
        t = net.t.cpu().numpy().reshape(B, -1)
        hole = ~np.isfinite(t)
        assert (0.02 < hole.mean() < 0.5) if holes else not hole.any()
        scalars = net.summary_scalars(out)
        for which, quad in (('coarse', net.loss_berhu_c), ('fine', net.loss_berhu_f)):
            o = getattr(net, which).cpu().numpy().reshape(B, -1)
            l64, g64, b_loss, b_grad = R.bound(o, t, masked, FRACTION)
            got = quad.cpu().numpy()
            e_loss, e_c = R.rel(got[0], l64[0]), R.rel(got[2], l64[2])
            print(f'{which} start {start} holes {holes}: loss {e_loss:.2e} threshold {e_c:.2e} (bound {b_loss:.2e}); loss '
                  f'{l64[0]:.6g} threshold {l64[2]:.6g} quadratic {l64[3]:.4g}')
            assert np.isfinite(got).all() and b_loss > 0 and e_loss <= b_loss and e_c <= b_loss
            assert got[1] == np.float32((~hole).mean())
            total = int((~hole).sum())
            assert abs(float(got[3]) * total - l64[3] * total) <= R.ambiguous(o, t, masked, FRACTION) + 0.5 and 0 < got[3] < 1
            # the summary scalars are the buffers' values
            assert float(out[which + '_loss']) == got[0] and scalars[f'loss/{which}_loss'] == float(got[0])
            assert scalars[f'loss/{which}_threshold'] == float(got[2]) and scalars[f'loss/{which}_quadratic'] == float(got[3])
            if which != ('coarse' if start == 0 else 'fine'):
                continue
            g = (net.dz1 if start == 0 else net.dfine).cpu().numpy().reshape(B, -1)
            e_grad = R.grad_err(g, g64)
            print(f'  d{which}: {e_grad:.2e} (bound {b_grad:.2e})')
            assert b_grad > 0 and e_grad <= b_grad and np.isfinite(g).all()
            assert (g[hole].view(np.uint32) == 0).all() and (g[~hole & (o != t)] != 0).all()
            # against the log loss on the same tensors: another gradient, and one that reaches the outputs at or below zero.
            # On the replica's own outputs first, then shifted by their median, so that half lie there whatever the weights give.
            own = getattr(net, which).reshape(B, -1)
            for name, outs, want in (('own', own, g), ('shifted', (own - own.median()).contiguous(), None)):
                oh = outs.cpu().numpy()
                log_g, berhu_g = torch.empty((B, 4070), device='cuda'), torch.empty((B, 4070), device='cuda')
                loss4 = torch.empty(4, device='cuda')
                ws = (ops.silog_masked_ws if holes else ops.silog_ws)(B, 'cuda')
                if holes:
                    ops.silog_masked_loss_fwd(outs, net.t, loss4[:2], ws)
                    ops.silog_masked_loss_bwd(outs, net.t, ws, log_g)
                else:
                    ops.silog_loss_fwd(outs, net.t, loss4[:1], ws)
                    ops.silog_loss_bwd(outs, net.t, ws, log_g)
                wsh = ops.berhu_ws(B, 'cuda')
                ops.berhu_loss_fwd(outs, net.t, masked, FRACTION, loss4, wsh)
                ops.berhu_loss_bwd(outs, net.t, masked, FRACTION, wsh, berhu_g)
                torch.cuda.synchronize()
                log_g, berhu_g = log_g.cpu().numpy(), berhu_g.cpu().numpy()
                assert want is None or np.array_equal(berhu_g.view(np.uint32), want.view(np.uint32))   # the step's own launch
                assert rel_l2(berhu_g, log_g) > 0.1
                below = ~hole & (oh < -1e-8)                                 # log(o + 1e-8) is NaN there
                print(f'  {name} outputs: {int(below.sum())} below zero')
                assert below.sum() > (1000 if want is None else 0)
                assert (log_g[below] == 0).all() and (berhu_g[~hole & (oh <= 0) & (oh != t)] != 0).all()
        assert ('valid_fraction' in scalars) == holes and set(NEW_TAGS) <= set(scalars)
    for gname in net.groups:
        assert bool(torch.isfinite(net.groups[gname].var).all()), gname


def test_bf16_storage_takes_the_gradient_as_bf16_rows(params):
    from ann3depth_amd import models
    img, dep, keep = stored_batch(5, holes=True)
    net = models.MSDNReplica(B, params=params, beta2=0.999, precision='bf16s', valid_range=(0, INF), objective='berhu')
    out = net.step(dev(img), dev(dep), dev(keep))
    torch.cuda.synchronize()
    assert np.isfinite(float(out['coarse_loss'])) and np.isfinite(float(out['fine_loss'])) and float(net.loss_berhu_c[2]) > 0
    dz1, dz16 = net.dz1.cpu(), net.dz1_16.float().cpu()
    assert torch.equal(dz16[:, :4070], dz1.to(torch.bfloat16).float()) and bool((dz16[:, 4070:] == 0).all())
    hole = ~np.isfinite(net.t.cpu().numpy().reshape(B, -1))
    assert hole.any() and bool((dz1.numpy()[hole] == 0).all()) and bool((dz1 != 0).any())


def test_bad_objectives_are_refused(params):
    from ann3depth_amd import models
    with pytest.raises(ValueError, match='objective'):
        models.MSDNReplica(B, params=params, objective='l2')
    for bad in (0.0, -0.2, 1.5, float('nan')):
        with pytest.raises(ValueError, match='berhu_fraction'):
            models.MSDNReplica(B, params=params, objective='berhu', berhu_fraction=bad)
    with pytest.raises(ValueError, match='grad_weight'):
        models.MSDNReplica(B, params=params, objective='berhu', grad_weight=0.5)
    assert models.msdn.objective == 'silog' and models.msdn.berhu_fraction == 0.2


# ---------------------------------------------------------------------------------------------- the drivers
def losses(ck, run):
    return {r['global_step']: (r['loss/coarse_loss'], r['loss/fine_loss']) + tuple(r.get(tag) for tag in NEW_TAGS)
            for r in rows(ck, run)}


def restore_signals():
    for s in (signal.SIGUSR1, signal.SIGUSR2, signal.SIGALRM, signal.SIGINT, signal.SIGTERM):
        signal.signal(s, signal.SIG_DFL)


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
    """A shard with holes (the same records as its test split) and run `a`: four steps under --loss berhu, shared by the two
    driver tests below."""
    from ann3depth_amd import models
    root = tmp_path_factory.mktemp('berhu')
    data, ck = str(root / 'holed'), str(root / 'ckpt')
    write_shard(data, holes=True)
    shutil.copy(os.path.join(data, 'nyu', 'train.tfrecords'), os.path.join(data, 'nyu', 'test.tfrecords'))
    try:
        a = train(ck, data, 'a', 4, '--loss', 'berhu')
        assert models.msdn.objective == 'berhu' and models.msdn.berhu_fraction == 0.2
    finally:
        reset_plugin()
    return ck, data, a


def test_driver_under_berhu_is_reproducible_and_resumable(trained):
    from ann3depth_amd import models
    ck, data, a = trained
    try:
        assert sorted(a) == [1, 2, 3, 4]
        assert all(v is not None and np.isfinite(v) for six in a.values() for v in six) and len(set(a.values())) == 4
        first = train(ck, data, 'c', 2, '--loss', 'berhu')
        resumed = train(ck, data, 'c', 4, '--loss', 'berhu')               # continues from the step-2 checkpoint
        assert first == {k: a[k] for k in (1, 2)} and resumed == a        # a second run, and a resumed one: the same values
        for col, tag in enumerate(NEW_TAGS, start=2):
            logged = event_scalars(ck, 'msdn_a', tag)
            assert logged == [float(np.float32(a[k][col])) for k in sorted(a)] and all(v > 0 for v in logged)
        assert len(event_scalars(ck, 'msdn_a', 'valid_fraction')) == 4     # stays as it is
        half = train(ck, data, 'd', 1, '--loss', 'berhu', '--berhu-fraction', '0.5')
        assert models.msdn.berhu_fraction == 0.5 and half[1][2] > a[1][2] and half[1][4] < a[1][4]
        # the default: the scale-invariant log loss, and no new tag
        without = train(ck, data, 'f', 1)
        assert models.msdn.objective == 'silog' and all(v is None for v in without[1][2:]) and without[1][:2] != a[1][:2]
        assert not any(tag in r for tag in NEW_TAGS for r in rows(ck, 'msdn_f'))
        for tag in NEW_TAGS:
            assert event_scalars(ck, 'msdn_f', tag) == []
    finally:
        reset_plugin()


def test_evaluate_reports_berhu_only_when_asked(trained, capsys):
    """The checkpoint of the berHu run restores wherever an MSDN checkpoint does; `berhu` appears beside `silog` with the flag."""
    from ann3depth_amd import evaluate
    ck, data, _ = trained
    base = ['--model', 'msdn', '--batchsize', '4', '--ckptdir', ck, '--datadir', data, '--id', 'a']
    capsys.readouterr()
    assert evaluate.main(base + ['nyu']) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert evaluate.main(base + ['--loss', 'berhu', 'nyu']) == 0
    got = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert evaluate.main(base + ['--loss', 'berhu', '--berhu-fraction', '1', 'nyu']) == 0
    l1 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert plain['global_step'] == 4 and set(got) - set(plain) == {'loss', 'berhu_fraction'}
    assert (got['loss'], got['berhu_fraction'], l1['berhu_fraction']) == ('berhu', 0.2, 1.0)
    for name in ('coarse', 'fine'):
        assert 'berhu' not in plain[name] and set(got[name]) - set(plain[name]) == {'berhu'}
        assert np.isfinite(got[name]['berhu']) and got[name]['berhu'] > l1[name]['berhu'] > 0          # rho >= |e|
        for k in plain[name]:
            assert json.dumps(got[name][k]) == json.dumps(plain[name][k]), (name, k)
    # refused before any GPU work
    assert evaluate.main(['--model', 'dcnf', '--ckptdir', ck, '--datadir', data, '--loss', 'berhu', 'nyu']) == 2
    for bad in ('0', '1.5', 'nan'):
        assert evaluate.main(base + ['--loss', 'berhu', '--berhu-fraction', bad, 'nyu']) == 2
    assert evaluate.main(base + ['--berhu-fraction', '0.5', 'nyu']) == 2


def test_cli_refusals_come_before_anything_is_set_up(tmp_path):
    from ann3depth_amd import ann3depth
    try:
        common = ['--ckptdir', str(tmp_path), '--datadir', str(tmp_path)]
        assert ann3depth.main(['--model', 'dcnf', *common, '--loss', 'berhu', 'nyu']) == 2
        assert ann3depth.main(['--model', 'msdn', *common, '--loss', 'berhu', '--loss-gradient', '0.5', 'nyu']) == 2
        assert ann3depth.main(['--model', 'msdn', *common, '--loss', 'berhu', '--loss-gradient', '0', 'nyu']) == 2
        assert ann3depth.main(['--model', 'msdn', *common, '--berhu-fraction', '0.5', 'nyu']) == 2
        assert ann3depth.main(['--model', 'msdn', *common, '--loss', 'silog', '--berhu-fraction', '0.5', 'nyu']) == 2
        for bad in ('0', '-0.2', '1.5', 'nan'):
            assert ann3depth.main(['--model', 'msdn', *common, '--loss', 'berhu', '--berhu-fraction', bad, 'nyu']) == 2
        assert not os.listdir(tmp_path)                                    # refused before anything was set up
    finally:
        restore_signals()
