"""models.DCNFReplica(train_pairwise=True) and `--train-pairwise` on the GPU: the pairwise dense layer's gradient and its
floored descent step against float64 computed on the host from the replica's own z, y and sims; the unary group
untouched by the flag; the flag off leaving the layer where it was; descent of the layer alone on a fixed batch; two
ranks; the driver; a checkpoint.  Batch 2.

The replica's initial z is an untrained network's; against a random target the energy saturates the loss at -log(eps)
and every gradient is 1e-7 of itself.  batch_for() therefore builds the target from the replica's own z (superpixel
means z + noise of 0.05, as crf_loss_ref's draws do), and start_params() starts the layer at ((1, 1), 1): a live loss
and a gradient of both signs."""
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
import dcnf_pair_ref as P
from oracle import dcnf as OD

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
KERNEL, BIAS = OD.PAIR_PREFIX + 'kernel', OD.PAIR_PREFIX + 'bias'
# r = sims w + b lies in [1, 3] here, between and above the ranges of the two measured 6x8 regimes that do not exchange
# rows ('reference' [-0.1, 0.7], 'unsaturated' [2, 2.3]): the larger of their two bounds
DR_BOUND = max(G.bound(6, 8, 'reference'), G.bound(6, 8, 'unsaturated'))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def start_params(w=(1.0, 1.0), b=1.0):
    params = OD.init_params(3000)
    params[KERNEL], params[BIAS] = np.array(w, F).reshape(2, 1), np.array([b], F)
    return params


def batch_for(rep, B, seed):
    """(images [B, 240, 320, 3], depths [B, 240, 320, 1]) on the device: dcnf_pair_ref's images (both similarities inside
    (0, 1) in the first two) and a target whose superpixel means are the replica's current z plus noise."""
    img = torch.from_numpy(P.image(240, 320, 40, B, seed=seed)).cuda()
    rep.unary.forward(img)
    z = rep.unary.z.view(B, rep.rows, rep.cols).cpu().numpy()
    y = (z + 0.05 * np.random.default_rng(seed).standard_normal(z.shape)).astype(F)
    dep = np.kron(y, np.ones((40, 40), F))[..., None]
    return img, torch.from_numpy(np.ascontiguousarray(dep)).cuda()


def host_gradient(rep):
    """float64 on the host from what the replica holds: (dw [2], db, sum |dr| |sims| [2], sum |dr|)."""
    B = rep.B
    z, y = rep.unary.z.view(B, 48).cpu().numpy(), rep.y.view(B, 48).cpu().numpy()
    sims, r = rep.sims.cpu().numpy().astype(np.float64), rep.r.cpu().numpy()
    dr64 = G.grad64(z, y, r, *L.pairs(6, 8))
    dw, db = G.dense_bwd64(sims, dr64)
    return dw, db, np.einsum('bq,bqk->k', np.abs(dr64), np.abs(sims)), np.abs(dr64).sum()


def test_one_step_moves_the_pairwise_layer_as_float64_says_and_the_unary_group_as_before():
    from ann3depth_amd import models
    B, params = 2, start_params()
    rep = models.DCNFReplica(B, params=params, train_pairwise=True)
    img, dep = batch_for(rep, B, seed=21)
    before = rep.pair_group.var.clone()
    out = rep.step(img, dep)
    torch.cuda.synchronize()
    assert rep.global_step == 1 and float(out['mean_loss']) < 15.5
    dw64, db64, abs_w, abs_b = host_gradient(rep)
    gw, gb = rep.pair_grad('kernel').cpu().numpy().reshape(2), float(rep.pair_grad('bias'))
    print(f'dcnf pairwise step: dw {gw} (float64 {dw64}, |err| {np.abs(gw - dw64)}, bound {DR_BOUND * abs_w}), '
          f'db {gb} (float64 {db64}, |err| {abs(gb - db64):.3g}, bound {DR_BOUND * abs_b:.3g}), loss {float(out["mean_loss"]):.4f}')
    assert (np.abs(dw64) > 1e-3).all() and abs(db64) > 1e-3
    assert (np.abs(gw - dw64) <= DR_BOUND * abs_w).all() and abs(gb - db64) <= DR_BOUND * abs_b
    # the step: fl(var - fl(0.1 g)) floored at 0, from the kernel's own gradient bit for bit; from float64's within 0.1 of
    # the gradient's bound and the two roundings of the update
    after = rep.pair_group.var.cpu().numpy()
    np.testing.assert_array_equal(bits(after), bits(G.sgd_floor32(before.cpu().numpy(), rep.pair_group.grad.cpu().numpy(), 0.1, 0.0)))
    w1, b1 = rep.pair_var('kernel').cpu().numpy().reshape(2).astype(np.float64), float(rep.pair_var('bias'))
    want_w, want_b = 1.0 - 0.1 * dw64, 1.0 - 0.1 * db64
    assert (want_w > 0).all() and want_b > 0
    assert (np.abs(w1 - want_w) <= 0.1 * DR_BOUND * abs_w + 2 * L.U * (1 + 0.1 * np.abs(dw64))).all()
    assert abs(b1 - want_b) <= 0.1 * DR_BOUND * abs_b + 2 * L.U * (1 + 0.1 * abs(db64))
    assert (after >= 0).all() and (after[2:64] == 0).all() and (after[65:] == 0).all()       # the padding stays zero
    # the same inputs and pairwise values without the flag: the unary group cannot tell
    off = models.DCNFReplica(B, params=params)
    out_off = off.step(img, dep)
    torch.cuda.synchronize()
    assert off.dr is None and torch.equal(off.pair_group.grad, torch.zeros_like(off.pair_group.grad))
    for a, b in ((out['mean_loss'], out_off['mean_loss']), (rep.dz, off.dz), (rep.r, off.r),
                 (rep.unary.group.grad, off.unary.group.grad), (rep.unary.group.var, off.unary.group.var)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert float(rep.unary.group.grad.abs().max()) > 0


def test_without_the_flag_the_pairwise_layer_stays_where_it_was():
    from ann3depth_amd import models
    params = start_params(w=(-0.5, 0.75), b=0.25)                          # values the projection would have changed
    rep = models.DCNFReplica(2, params=params)
    assert rep.train_pairwise is False
    img, dep = batch_for(rep, 2, seed=4)
    before = rep.pair_group.var.clone()
    for _ in range(3):
        rep.step(img, dep)
    torch.cuda.synchronize()
    assert rep.global_step == 3
    assert torch.equal(rep.pair_group.var.view(torch.int32), before.view(torch.int32))
    np.testing.assert_array_equal(bits(rep.pair_var('kernel').cpu().numpy()), bits(params[KERNEL]))
    on = models.DCNFReplica(2, params=params, train_pairwise=True)          # construction projects once
    np.testing.assert_array_equal(bits(on.pair_var('kernel').cpu().numpy()), bits(np.maximum(params[KERNEL], 0)))


def test_descent_of_the_layer_alone_on_a_fixed_batch_follows_float64():
    """pair_similarity -> crf_loss_grad -> pair_dense_bwd -> sgd_apply_floor, ten times from ((1, 1), 1) on five images
    of dcnf_pair_ref.image and the z, y of crf_loss_ref's 'unsaturated' batch of 5.  The loss decreases strictly; every
    step lands within the propagated bound of the float64 step from the same point (0.1 x the dr bound x the host sum of
    |dr| |sims|, plus the update's two roundings), and so the ten steps stay near the float64 run from the start: errors
    fed back through the descent are not bounded by one step's, they are printed and held to ten times the summed bound."""
    from ann3depth_amd import ops
    left, right = L.pairs(6, 8)
    li, ri = (torch.tensor(np.asarray(a, np.int32)).cuda() for a in (left, right))
    x = torch.from_numpy(P.image(240, 320, 40, 5)).cuda()
    z, y, _ = (torch.from_numpy(a.copy()).cuda() for a in L.draw(6, 8, 5, 'unsaturated'))
    hist = ops.superpixel_hist(x, 40)
    var, grad = torch.zeros(128, device='cuda'), torch.zeros(128, device='cuda')
    var[0], var[1], var[64] = 1.0, 1.0, 1.0
    losses, summed = [], np.zeros(3)
    for it in range(10):
        sims, r = ops.pair_similarity(x, 40, hist, li, ri, var[:2].view(2, 1), var[64:65], 1.0)
        mean, _, _, dr = ops.crf_loss_grad(z, y, r, li, ri, L.EPSILON)
        ops.pair_dense_bwd(sims, dr, grad[:2].view(2, 1), grad[64:65])
        at = var.cpu().numpy().astype(np.float64)
        ops.sgd_apply_floor(var, grad, 0.1, 0.0)
        losses.append(float(mean))
        s64 = sims.cpu().numpy().astype(np.float64)
        dr64 = G.grad64(z.cpu().numpy(), y.cpu().numpy(), r.cpu().numpy(), left, right)
        dw64, db64 = G.dense_bwd64(s64, dr64)
        g64 = np.array([dw64[0], dw64[1], db64])
        step_bound = 0.1 * DR_BOUND * np.append(np.einsum('bq,bqk->k', np.abs(dr64), s64), np.abs(dr64).sum()) + \
            2 * L.U * (np.abs(at[[0, 1, 64]]) + 0.1 * np.abs(g64))
        got = var.cpu().numpy()[[0, 1, 64]].astype(np.float64)
        err = np.abs(got - np.maximum(at[[0, 1, 64]] - 0.1 * g64, 0))
        summed += step_bound
        print(f'  step {it}: loss {losses[-1]:.6f}, (w, b) {got}, |err| {err}, bound {step_bound}')
        assert (err <= step_bound).all()
    l64, path = G.descend64(z.cpu().numpy(), y.cpu().numpy(), s64, left, right, (1.0, 1.0), 1.0, 10)
    end64 = np.append(path[-1][0], path[-1][1])
    print(f'descent: losses {losses}, float64 {l64}; ends at {got}, float64 {end64}, summed bound {summed}')
    assert (np.diff(losses) < 0).all() and max(losses) < 15.5
    assert (np.abs(got - end64) <= 10 * summed).all() and (got >= 0).all()
    # the loss itself: crf_loss_ref's 6x8 bounds at the same point, and the two runs' points differ by far less
    assert np.abs(np.array(losses) / l64 - 1).max() <= 2 * max(L.bound(6, 8, 'reference')[0], L.bound(6, 8, 'unsaturated')[0])


def test_two_ranks_keep_the_pairwise_weights_bit_identical(tmp_path):
    """tests/dcnf_pair_dp_worker.py: two ranks on the one GPU over gloo, another batch on each."""
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / 'ok.txt')
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), A3D_DIST_BACKEND='gloo')
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, 'dcnf_pair_dp_worker.py'), out], env=env))
    for p in procs:
        assert p.wait(timeout=300) == 0
    assert open(out).read() == '1'


def test_the_driver_trains_the_pairwise_layer_of_dcnf_and_of_nothing_else(tmp_path):
    """Eight records whose depth maps are built from what the driver's initial network (its fixed seed) answers on their
    images, so that the loss is live and the layer has something to learn from; see batch_for()."""
    from ann3depth_amd import ann3depth, models, tfrecord
    root = str(tmp_path / 'data')
    os.makedirs(os.path.join(root, 'nyu'))
    probe = models.DCNFReplica(2)
    with tfrecord.TFRecordWriter(os.path.join(root, 'nyu', 'train.tfrecords')) as w:
        for i in range(4):
            img, dep = batch_for(probe, 2, seed=30 + i)
            for b in range(2):
                w.write_example(img[b].cpu().numpy() - F(0.5), dep[b].cpu().numpy() - F(0.5))      # the loader adds 0.5
    del probe
    ck = str(tmp_path / 'ckpt')
    common = ['nyu', '--steps', '3', '--batchsize', '2', '--datadir', root, '--ckptdir', ck, '--sumfreq', '1', '--ckptfreq', '0']
    try:
        assert ann3depth.main(common + ['--model', 'msdn', '--train-pairwise']) == 2
        assert not os.path.exists(os.path.join(ck, 'msdn'))
        assert ann3depth.main(common + ['--model', 'dcnf', '--train-pairwise']) == 0
        assert models.dcnf.train_pairwise is True
    finally:
        models.dcnf.train_pairwise = False
    d = os.path.join(ck, 'dcnf')
    recs = [json.loads(l) for l in open(os.path.join(d, 'summaries.jsonl'))]
    assert [r['global_step'] for r in recs] == [1, 2, 3] and all(np.isfinite(r['loss/mean_loss']) for r in recs)
    sd = torch.load(os.path.join(d, 'model.ckpt-3.pt'))
    start = models.DCNFReplica(2, train_pairwise=True)                      # the driver's seed: the projected initial draw
    moved = [not torch.equal(sd[n].cpu(), start.pair_var(n.rsplit('/', 1)[1]).cpu()) for n in (KERNEL, BIAS)]
    print(f'driver: kernel {sd[KERNEL].reshape(-1).tolist()}, bias {sd[BIAS].tolist()}, started at '
          f'{start.pair_var("kernel").reshape(-1).tolist()}')
    print(f'driver: losses {[r["loss/mean_loss"] for r in recs]}')
    assert moved[0] and float(sd[KERNEL].min()) >= 0 and float(sd[BIAS].min()) >= 0      # (a bias at the floor may rest there)
    assert ann3depth.main(common + ['--model', 'dcnf', '--steps', '4']) == 0      # resumed without the flag: the layer rests
    sd4 = torch.load(os.path.join(d, 'model.ckpt-4.pt'))
    assert int(sd4['global_step']) == 4 and torch.equal(sd4[KERNEL], sd[KERNEL]) and torch.equal(sd4[BIAS], sd[BIAS])


def test_a_checkpoint_written_then_restored_gives_the_same_bits():
    from ann3depth_amd import models
    rep = models.DCNFReplica(2, params=start_params(), train_pairwise=True)
    img, dep = batch_for(rep, 2, seed=8)
    rep.step(img, dep)
    sd = {k: v.clone() for k, v in rep.state_dict().items()}
    tf = rep.tf_variables()
    assert not np.array_equal(tf[KERNEL], start_params()[KERNEL])
    a, b = models.DCNFReplica(2, seed=1, train_pairwise=True), models.DCNFReplica(2, seed=2, train_pairwise=True)
    a.load_state_dict(sd)
    b.load_tf_variables(tf)
    for other in (a, b):
        assert other.global_step == 1
        for g, h in zip(rep.groups.values(), other.groups.values()):
            assert torch.equal(g.var.view(torch.int32), h.var.view(torch.int32))
    rep.step(img, dep)
    a.step(img, dep)
    torch.cuda.synchronize()
    assert torch.equal(rep.pair_group.var.view(torch.int32), a.pair_group.var.view(torch.int32))
    assert torch.equal(rep.loss.view(torch.int32), a.loss.view(torch.int32))
