"""models.DCNFReplica(pairwise_texture=True) and `--pairwise-texture` on the GPU: the three kernel gradients and the bias
gradient of one step against float64 on the host, under the rule of tests/test_gpu_dcnf_pairwise_train.py (its DR_BOUND,
its batch_for(): a target built from the replica's own z so that the loss is live); the argument off leaving every bit
where a default replica puts it; two ranks; the driver, its checkpoints in both forms, evaluation of a three- and of a
two-feature checkpoint; the refusals.  Batch 2."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import crf_loss_ref as L
import crf_pair_grad_ref as G
import texture_ref as T
from oracle import dcnf as OD
from test_gpu_dcnf_pairwise_train import BIAS, DR_BOUND, KERNEL, batch_for, bits

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32


def start_params3(w=(1.0, 0.5, 0.5), b=1.0):
    """The layer at ((1, 1/2, 1/2), 1): r = sims w + b stays in [1, 3], the range DR_BOUND was chosen for."""
    params = OD.init_params(3000)
    params[KERNEL], params[BIAS] = np.array(w, F).reshape(3, 1), np.array([b], F)
    return params


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_one_step_moves_the_three_weights_as_float64_says():
    from ann3depth_amd import models
    B, params = 2, start_params3()
    rep = models.DCNFReplica(B, params=params, train_pairwise=True, pairwise_texture=True)
    assert tuple(rep.pair_var('kernel').shape) == (3, 1) and tuple(rep.lbp.shape) == (B, 48, 256)
    img, dep = batch_for(rep, B, seed=21)
    before = rep.pair_group.var.clone()
    out = rep.step(img, dep)
    torch.cuda.synchronize()
    assert rep.global_step == 1 and float(out['mean_loss']) < 15.5
    assert tuple(rep.sims.shape) == (B, 48, 3)
    # the forward the step ran: the LBP counts of the resized batch, the texture similarity they give
    x = rep.unary.resized.cpu().numpy()
    assert torch.equal(rep.lbp.cpu(), torch.from_numpy(T.lbp_histogram(x, 40)))
    left, right = L.pairs(6, 8)
    sims = rep.sims.cpu().numpy()
    s64, _ = T.similarity3_64(x, 40, rep.hist.cpu().numpy(), rep.lbp.cpu().numpy(), left, right, params[KERNEL],
                              params[BIAS], 1.0)
    import dcnf_pair_ref as P
    assert (P.rel_errors(sims[..., 2], s64[..., 2]) <= T.texture_bound(rep.lbp.cpu().numpy(), left, right, 1.0, 40)).all()
    assert 0 < sims[..., 2].min() and sims[..., 2].max() <= 1 and sims[..., 2].min() < 1
    r = rep.r.cpu().numpy()
    assert 1 <= r.min() and r.max() <= 3
    # the gradient: float64 on the host from the replica's own z, y, r and sims
    z, y = rep.unary.z.view(B, 48).cpu().numpy(), rep.y.view(B, 48).cpu().numpy()
    dr64 = G.grad64(z, y, r, left, right)
    dw64, db64 = G.dense_bwd64(sims, dr64)
    abs_w, abs_b = np.einsum('bq,bqk->k', np.abs(dr64), np.abs(sims.astype(np.float64))), np.abs(dr64).sum()
    gw, gb = rep.pair_grad('kernel').cpu().numpy().reshape(3), float(rep.pair_grad('bias'))
    print(f'dcnf texture step: dw {gw} (float64 {dw64}, |err| {np.abs(gw - dw64)}, bound {DR_BOUND * abs_w}), '
          f'db {gb} (float64 {db64}, |err| {abs(gb - db64):.3g}, bound {DR_BOUND * abs_b:.3g}), '
          f'loss {float(out["mean_loss"]):.4f}, texture similarity in [{sims[..., 2].min():.4f}, {sims[..., 2].max():.4f}]')
    assert (np.abs(dw64) > 1e-3).all() and abs(db64) > 1e-3
    assert (np.abs(gw - dw64) <= DR_BOUND * abs_w).all() and abs(gb - db64) <= DR_BOUND * abs_b
    # the step: fl(var - fl(0.1 g)) floored at 0 from the kernel's own gradient, bit for bit; the weights stay >= 0
    after = rep.pair_group.var.cpu().numpy()
    np.testing.assert_array_equal(bits(after), bits(G.sgd_floor32(before.cpu().numpy(), rep.pair_group.grad.cpu().numpy(), 0.1, 0.0)))
    assert (after >= 0).all() and (after[3:64] == 0).all() and (after[65:] == 0).all()       # the padding stays zero
    assert (after[[0, 1, 2, 64]] != before.cpu().numpy()[[0, 1, 2, 64]]).all()
    # a layer that starts below zero is projected at construction and stays >= 0
    neg = models.DCNFReplica(B, params=start_params3(w=(-0.5, 0.75, -0.25), b=-1.0), train_pairwise=True, pairwise_texture=True)
    np.testing.assert_array_equal(neg.pair_var('kernel').cpu().numpy().reshape(3), np.array([0, 0.75, 0], F))
    neg.step(img, dep)
    assert float(neg.pair_group.var.min()) >= 0


def test_without_the_texture_argument_every_bit_is_a_default_replicas():
    from ann3depth_amd import models
    for kw in ({}, {'train_pairwise': True}):
        a = models.DCNFReplica(2, seed=5, **kw)
        b = models.DCNFReplica(2, seed=5, pairwise_texture=False, **kw)
        assert not hasattr(b, 'lbp') and tuple(b.pair_var('kernel').shape) == (2, 1)
        assert same_bits(a.pair_group.var, b.pair_group.var)
        img, dep = batch_for(a, 2, seed=9)
        oa, ob = a.step(img, dep), b.step(img, dep)
        torch.cuda.synchronize()
        assert tuple(b.sims.shape) == (2, 48, 2)
        for u, v in ((oa['mean_loss'], ob['mean_loss']), (a.dz, b.dz), (a.sims, b.sims), (a.r, b.r),
                     (a.unary.group.var, b.unary.group.var), (a.unary.group.grad, b.unary.group.grad),
                     (a.pair_group.var, b.pair_group.var)):
            assert same_bits(u, v)
        assert float(a.unary.group.grad.abs().max()) > 0
    # with it, the first two similarities of the same batch are the same bits and only r differs
    c = models.DCNFReplica(2, seed=5, pairwise_texture=True)
    c.forward(img, dep)
    assert same_bits(c.sims[..., :2], a.sims) and tuple(c.pair_var('kernel').shape) == (3, 1)
    want = models.glorot_uniform(np.random.default_rng(5 + 1), (3, 1))     # the same stream as the two-feature draw
    np.testing.assert_array_equal(bits(c.pair_var('kernel').cpu().numpy()), bits(want))


def test_two_ranks_keep_the_four_pairwise_values_bit_identical(tmp_path):
    """tests/texture_dp_worker.py: two ranks on the one GPU over gloo, another batch on each."""
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / 'ok.txt')
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), A3D_DIST_BACKEND='gloo')
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, 'texture_dp_worker.py'), out], env=env))
    for p in procs:
        assert p.wait(timeout=300) == 0
    assert open(out).read() == '1'


def _write_records(path, probe, count, seed):
    """Records whose depth maps are built from what the driver's initial network answers on their images (batch_for)."""
    from ann3depth_amd import tfrecord
    with tfrecord.TFRecordWriter(path) as w:
        for i in range(count // 2):
            img, dep = batch_for(probe, 2, seed=seed + i)
            for b in range(2):
                w.write_example(img[b].cpu().numpy() - F(0.5), dep[b].cpu().numpy() - F(0.5))      # the loader adds 0.5


def test_the_driver_writes_a_three_feature_checkpoint_and_evaluate_reads_it(tmp_path, capsys):
    from ann3depth_amd import ann3depth, evaluate, models, tfckpt
    root = str(tmp_path / 'data')
    os.makedirs(os.path.join(root, 'nyu'))
    probe = models.DCNFReplica(2)
    _write_records(os.path.join(root, 'nyu', 'train.tfrecords'), probe, 8, 30)
    _write_records(os.path.join(root, 'nyu', 'test.tfrecords'), probe, 4, 40)
    del probe
    ck = str(tmp_path / 'ckpt')
    common = ['nyu', '--steps', '3', '--batchsize', '2', '--datadir', root, '--ckptdir', ck, '--sumfreq', '1', '--ckptfreq', '0']
    try:
        assert ann3depth.main(common + ['--model', 'msdn', '--pairwise-texture']) == 2
        assert not os.path.exists(os.path.join(ck, 'msdn'))
        assert ann3depth.main(common + ['--model', 'dcnf', '--train-pairwise', '--pairwise-texture', '--tf-checkpoints']) == 0
        assert models.dcnf.train_pairwise is True and models.dcnf.pairwise_texture is True
        # a two-feature run beside it, for evaluate and for the refusals
        assert ann3depth.main(common + ['--model', 'dcnf', '--id', 'two', '--steps', '1']) == 0
        assert models.dcnf.pairwise_texture is False
        # resuming across the flag is refused, both ways, with both shapes in the message
        with pytest.raises(ValueError, match=r'has shape \[3, 1\], this replica.s is \[2, 1\]'):
            ann3depth.main(common + ['--model', 'dcnf', '--steps', '4'])
        with pytest.raises(ValueError, match=r'has shape \[2, 1\], this replica.s is \[3, 1\]'):
            ann3depth.main(common + ['--model', 'dcnf', '--id', 'two', '--steps', '2', '--pairwise-texture'])
    finally:
        models.dcnf.train_pairwise = False
        models.dcnf.pairwise_texture = False
    capsys.readouterr()
    d = os.path.join(ck, 'dcnf')
    recs = [json.loads(l) for l in open(os.path.join(d, 'summaries.jsonl'))]
    assert [r['global_step'] for r in recs] == [1, 2, 3] and all(np.isfinite(r['loss/mean_loss']) for r in recs)
    sd = torch.load(os.path.join(d, 'model.ckpt-3.pt'))
    assert tuple(sd[KERNEL].shape) == (3, 1) and float(sd[KERNEL].min()) >= 0 and float(sd[BIAS].min()) >= 0
    start = models.DCNFReplica(2, train_pairwise=True, pairwise_texture=True)          # the driver's seed
    assert not torch.equal(sd[KERNEL].cpu(), start.pair_var('kernel').cpu())           # the layer moved
    bundle = tfckpt.read_bundle(os.path.join(d, 'model.ckpt-3'))
    assert bundle[KERNEL].shape == (3, 1)
    np.testing.assert_array_equal(bits(bundle[KERNEL]), bits(sd[KERNEL].cpu().numpy()))
    # both forms restore to the same bits
    a = models.DCNFReplica(2, seed=1, pairwise_texture=True)
    b = models.DCNFReplica(2, seed=2, pairwise_texture=True)
    a.load_state_dict(sd)
    b.load_tf_variables(bundle)
    for g, h in zip(a.groups.values(), b.groups.values()):
        assert same_bits(g.var, h.var)
    assert a.global_step == b.global_step == 3
    # evaluate picks the feature count from the checkpoint
    base = ['--model', 'dcnf', '--batchsize', '2', '--ckptdir', ck, '--datadir', root]
    assert evaluate.main(base + ['nyu']) == 0
    got = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert got['pairwise_texture'] is True and got['records'] == 4 and got['global_step'] == 3
    assert np.isfinite(got['crf_nll']) and got['singular_systems'] == 0
    assert evaluate.main(base + ['--checkpoint', os.path.join(d, 'model.ckpt-3'), 'nyu']) == 0
    got_tf = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert got_tf['pairwise_texture'] is True and got_tf['crf'] == got['crf'] and got_tf['crf_nll'] == got['crf_nll']
    assert evaluate.main(base + ['--id', 'two', 'nyu']) == 0
    two = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert 'pairwise_texture' not in two and two['records'] == 4 and two['global_step'] == 1
    # any other kernel shape: exit 2 with a message
    sd[KERNEL] = torch.zeros((4, 1))
    odd = str(tmp_path / 'odd.pt')
    torch.save(sd, odd)
    assert evaluate.main(base + ['--checkpoint', odd, 'nyu']) == 2
    assert '[4, 1]' in capsys.readouterr().err


def test_a_checkpoint_of_the_other_shape_is_refused_at_restore():
    from ann3depth_amd import models
    two, three = models.DCNFReplica(2), models.DCNFReplica(2, pairwise_texture=True)
    for src, dst, pattern in ((two, three, r'has shape \[2, 1\], this replica.s is \[3, 1\]'), (three, two, r'has shape \[3, 1\], this replica.s is \[2, 1\]')):
        before = dst.pair_group.var.clone()
        with pytest.raises(ValueError, match=pattern):
            dst.load_state_dict(src.state_dict())
        with pytest.raises(ValueError, match=pattern):
            dst.load_tf_variables(src.tf_variables())
        assert same_bits(dst.pair_group.var, before) and dst.global_step == 0            # nothing was copied
    with pytest.raises(ValueError, match=r'has shape \[2, 1\], this replica.s is \[3, 1\]'):
        models.DCNFReplica(2, params=two.tf_variables(), pairwise_texture=True)
    three.load_state_dict(models.DCNFReplica(2, seed=4, pairwise_texture=True).state_dict())      # its own shape loads
