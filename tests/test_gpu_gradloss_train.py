"""The MSDN training step and the driver with the gradient-matching term (MSDNReplica(grad_weight=...), --loss-gradient): at
weight 0 the step is today's step bit for bit; at weight 0.5 both totals, both gradient terms and the loss gradients are those of
tests/gradloss_ref.py on the replica's own outputs and target, with and without holes."""
import json
import os
import signal

import numpy as np
import pytest
import torch

import gradloss_ref as G
from oracle import msdn as O
from test_gpu_valid_train import event_scalars, fine_start, rows, stored_batch, write_shard

pytestmark = pytest.mark.gpu

INF = float('inf')
B = 2


@pytest.fixture(scope='module')
def params():
    return O.init_params(3000)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('valid_range', [None, (0, INF)])
def test_weight_zero_is_the_plain_step(params, valid_range):
    from ann3depth_amd import models
    img, dep, keep = stored_batch(1, holes=valid_range is not None)
    nets = [models.MSDNReplica(B, params=params, beta2=0.999, valid_range=valid_range),
            models.MSDNReplica(B, params=params, beta2=0.999, valid_range=valid_range, grad_weight=0.0)]
    assert nets[1].grad_weight == 0.0 and not hasattr(nets[1], 'loss_quad_c')
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


@pytest.mark.parametrize('holes', [False, True])
def test_step_with_the_term_is_the_reference(params, holes):
    from ann3depth_amd import models
    img, dep, keep = stored_batch(2, holes=holes)
    weight, masked = 0.5, int(holes)
    net = models.MSDNReplica(B, params=params, beta2=0.999, valid_range=(0.0, 0.99) if holes else None, grad_weight=weight)
    from ann3depth_amd import ops
    for start in (0, fine_start(models)):
        net.global_step = start
        out = net.step(dev(img), dev(dep), dev(keep))
        torch.cuda.synchronize()
        t = net.t.cpu().numpy().reshape(B, -1)
        hole = ~np.isfinite(t)
        assert (0.02 < hole.mean() < 0.5) if holes else not hole.any()
        scalars = net.summary_scalars(out)
        for which, quad in (('coarse', net.loss_quad_c), ('fine', net.loss_quad_f)):
            o = getattr(net, which).cpu().numpy().reshape(B, -1)
            refs, b_loss, b_grad = G.tolerances(o, t, 55, 74, masked)
            ref, g_ref = refs[weight]
            assert b_loss > 0 and b_grad > 0
            b_loss, b_grad = min(b_loss, 2e-6), min(b_grad, 1e-5)   # never looser than the masked loss's tolerances
            got = quad.cpu().numpy()
            errs = {k: G.rel(got[k], ref[k]) for k in (0, 2, 3)}
            print(f'{which} start {start} holes {holes}: total {errs[0]:.2e} silog {errs[2]:.2e} grad term {errs[3]:.2e} '
                  f'(bound {b_loss:.2e}); total {ref[0]:.6g} grad term {ref[3]:.6g}')
            assert np.isfinite(got).all() and max(errs.values()) <= b_loss
            assert float(out[which + '_loss']) == got[0] and got[1] == np.float32((~hole).mean()) and got[3] > 0
            assert scalars[f'loss/{which}_loss'] == float(got[0]) and scalars[f'loss/{which}_grad'] == float(got[3])
            # the silog part is the loss today's launch gives on the same tensors, bit for bit
            want, ws = torch.zeros(2, device='cuda'), (ops.silog_masked_ws if holes else ops.silog_ws)(B, 'cuda')
            if holes:
                ops.silog_masked_loss_fwd(getattr(net, which), net.t, want, ws)
            else:
                ops.silog_loss_fwd(getattr(net, which), net.t, want[:1], ws)
            assert got[2] == float(want[0])
            if which == ('coarse' if start == 0 else 'fine'):
                g = (net.dz1 if start == 0 else net.dfine).cpu().numpy().reshape(B, -1)
                e_grad = G.rel_l2(g, g_ref)
                print(f'  d{which}: rel-L2 {e_grad:.2e} (bound {b_grad:.2e})')
                assert e_grad <= b_grad and (g[hole] == 0).all() and np.isfinite(g).all() and (g != 0).any()
                plain_g = torch.empty((B, 4070), device='cuda')
                (ops.silog_masked_loss_bwd if holes else ops.silog_loss_bwd)(getattr(net, which), net.t, ws, plain_g)
                assert G.rel_l2(g, plain_g.cpu().numpy()) > 0.1                       # the term is in the gradient
        assert ('valid_fraction' in scalars) == holes
    for gname in net.groups:
        assert bool(torch.isfinite(net.groups[gname].var).all()), gname


def test_bf16_storage_takes_the_gradient_as_bf16_rows(params):
    from ann3depth_amd import models
    img, dep, keep = stored_batch(5, holes=True)
    net = models.MSDNReplica(B, params=params, beta2=0.999, precision='bf16s', valid_range=(0, INF), grad_weight=0.5)
    out = net.step(dev(img), dev(dep), dev(keep))
    torch.cuda.synchronize()
    assert np.isfinite(float(out['coarse_loss'])) and np.isfinite(float(out['fine_loss'])) and float(net.loss_quad_c[3]) > 0
    dz1, dz16 = net.dz1.cpu(), net.dz1_16.float().cpu()
    assert torch.equal(dz16[:, :4070], dz1.to(torch.bfloat16).float()) and bool((dz16[:, 4070:] == 0).all())
    hole = ~np.isfinite(net.t.cpu().numpy().reshape(B, -1))
    assert hole.any() and bool((dz1.numpy()[hole] == 0).all()) and bool((dz1 != 0).any())


def test_a_bad_weight_is_refused(params):
    from ann3depth_amd import models
    for bad in (-0.5, float('nan')):
        with pytest.raises(ValueError, match='grad_weight'):
            models.MSDNReplica(B, params=params, grad_weight=bad)


# ---------------------------------------------------------------------------------------------- the driver
def losses(ck, run):
    return {r['global_step']: (r['loss/coarse_loss'], r['loss/fine_loss'], r.get('loss/coarse_grad'), r.get('loss/fine_grad'))
            for r in rows(ck, run)}


def restore_signals():
    for s in (signal.SIGUSR1, signal.SIGUSR2, signal.SIGALRM, signal.SIGINT, signal.SIGTERM):
        signal.signal(s, signal.SIG_DFL)


def test_driver_with_the_term_is_reproducible_and_resumable(tmp_path):
    from ann3depth_amd import ann3depth, models
    data = tmp_path / 'holed'
    write_shard(str(data), holes=True)
    ck = str(tmp_path / 'ckpt')

    def run(run_id, steps, *flags):
        argv = ['--model', 'msdn', '--batchsize', '4', '--ckptdir', ck, '--datadir', str(data), '--sumfreq', '1',
                '--trace-every', '0', '--beta2', '0.999', '--min-depth', '0', '--id', run_id, '--steps', str(steps), *flags, 'nyu']
        assert ann3depth.main(argv) == 0
        return losses(ck, 'msdn_' + run_id)
    try:
        a = run('a', 6, '--loss-gradient', '0.5')
        assert models.msdn.grad_weight == 0.5
        b = run('b', 6, '--loss-gradient', '0.5')
        assert sorted(a) == [1, 2, 3, 4, 5, 6] and a == b                  # reproducible
        assert all(v is not None and np.isfinite(v) for four in a.values() for v in four) and len(set(a.values())) == 6
        first = run('c', 3, '--loss-gradient', '0.5')
        resumed = run('c', 6, '--loss-gradient', '0.5')                    # continues from the step-3 checkpoint
        assert first == {k: a[k] for k in (1, 2, 3)} and resumed == a
        for tag, col in (('loss/coarse_grad', 2), ('loss/fine_grad', 3)):
            logged = event_scalars(ck, 'msdn_a', tag)
            assert logged == [float(np.float32(a[k][col])) for k in sorted(a)] and all(v > 0 for v in logged)
        assert len(event_scalars(ck, 'msdn_a', 'valid_fraction')) == 6     # stays as it is
        # weight 0: the run without the flag, and no new tag
        zero = run('d', 3, '--loss-gradient', '0')
        assert models.msdn.grad_weight == 0.0
        without = run('e', 3)
        assert models.msdn.grad_weight == 0.0
        assert zero == without and all(four[2] is None and four[3] is None for four in zero.values())
        assert {k: v[:2] for k, v in zero.items()} != {k: a[k][:2] for k in (1, 2, 3)}
        for run_id in ('msdn_d', 'msdn_e'):
            assert not any('loss/coarse_grad' in r or 'loss/fine_grad' in r for r in rows(ck, run_id))
            assert event_scalars(ck, run_id, 'loss/coarse_grad') == [] and event_scalars(ck, run_id, 'loss/fine_grad') == []
    finally:
        models.msdn.valid_range = None
        models.msdn.grad_weight = 0.0
        models.msdn.beta2 = 1.0                  # --beta2 stays on the plugin; the tests after this one train without the flag
        restore_signals()


def test_dcnf_and_bad_weights_are_refused(tmp_path):
    from ann3depth_amd import ann3depth
    try:
        common = ['--ckptdir', str(tmp_path), '--datadir', str(tmp_path)]
        for w in ('0.5', '0'):
            assert ann3depth.main(['--model', 'dcnf', *common, '--loss-gradient', w, 'nyu']) == 2
        for w in ('-0.5', 'nan'):
            assert ann3depth.main(['--model', 'msdn', *common, '--loss-gradient', w, 'nyu']) == 2
        assert not os.listdir(tmp_path)                                    # refused before anything was set up
    finally:
        restore_signals()
