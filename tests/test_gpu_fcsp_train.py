"""`--unary fcsp` through the replica, the driver, checkpoints, evaluation and two ranks, at the model's size (240 x 320,
24 x 34 last map, 48 superpixels), B = 1 per replica.  The step is held to float64 on the host under the rules of
tests/test_gpu_dcnf.py::check_dcnf_train_step; everything after z is the patch form's code and is held to the patch
replica bit for bit given the same z."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import crf_loss_ref as L
import dcnf_pair_ref as P
import fcsp_ref as F
from oracle import dcnf as OD
from oracle import tf13_ops as T

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DENSE = OD.PREFIX + 'dense/kernel'


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def fcsp_params(seed=3000):
    params = F.init_params(seed)
    params.update(OD.pairwise_init(seed + 1))
    return params


def random_batch(B, seed):
    rng = np.random.default_rng(seed)
    img = (rng.integers(0, 256, (B, 480, 640, 3)) / 255).astype(np.float32)
    dep = rng.random((B, 55, 74, 1)).astype(np.float32)
    return img, dep


def test_fcsp_train_step_matches_float64_on_the_host():
    from ann3depth_amd import models
    B = 1
    img, dep = random_batch(B, 21)
    params = fcsp_params()
    rep = models.DCNFReplica(B, params=params, unary='fcsp')
    assert isinstance(rep.unary, models.DCNFUnaryFCSP) and rep.unary.map_hw == (24, 34) and rep.unary.P == 48
    before = {n: rep.unary.group.view(rep.unary.group.var, n).clone() for n in rep.unary.shapes}
    out = rep.step(torch.from_numpy(img).cuda(), torch.from_numpy(dep).cuda())
    torch.cuda.synchronize()
    assert rep.global_step == 1
    img240 = T.resize_bilinear_tf1(img, 240, 320)
    dep240 = T.resize_bilinear_tf1(dep, 240, 320)
    np.testing.assert_array_equal(rep.unary.resized.cpu().numpy(), img240)
    np.testing.assert_array_equal(rep.depths240.cpu().numpy(), dep240)
    r_gpu = rep.r.cpu().numpy()
    r64, _ = OD.pairwise_forward(params, img240.astype(np.float64))
    assert P.r_errors(r_gpu, r64[..., 0]).max() <= P.R_BOUND
    z_gpu = rep.unary.z.cpu().numpy().reshape(B, 48, 1)
    assert np.isfinite(z_gpu).all() and np.ptp(z_gpu) > 0
    m_ref, per_ref, dz_ref = OD.crf_loss(dep240.astype(np.float64), z_gpu.astype(np.float64), r_gpu.astype(np.float64)[..., None])
    b_loss, b_dz = L.bound(6, 8, 'reference')
    dz_gpu = rep.dz.cpu().numpy()
    e_loss, e_dz = L.errors(rep.loss_per_image.cpu().numpy(), dz_gpu, per_ref, dz_ref[..., 0])
    print(f'fcsp step: loss {e_loss.max():.3g} (bound {b_loss:.3g}), dz {e_dz.max():.3g} (bound {b_dz:.3g})')
    assert e_loss.max() <= b_loss and e_dz.max() <= b_dz
    np.testing.assert_allclose(float(out['mean_loss']), m_ref, rtol=b_loss + 16 * L.U)
    assert rel(dz_gpu, dz_ref[..., 0]) < b_dz * np.sqrt(48)
    # the backward chain in float64 on the activations the GPU produced, then var -= 0.1 * grad
    a = {k: v.astype(np.float64) for k, v in rep.unary.activations().items()}
    g = F.unary_backward({k: v.astype(np.float64) for k, v in params.items()}, a, dz_gpu.reshape(48, 1).astype(np.float64), 40)
    for n in rep.unary.shapes:
        ggpu = rep.unary.group.view(rep.unary.group.grad, n)
        if np.linalg.norm(g[n]) > 0:
            e = rel(ggpu.cpu().numpy(), g[n])
            print(f'{n}: rel-L2 {e:.3g}')
            assert e < 1e-4, n
        np.testing.assert_array_equal(rep.unary.group.view(rep.unary.group.var, n).cpu().numpy(),
                                      (before[n] - np.float32(0.1) * ggpu).cpu().numpy())
    assert sum(np.linalg.norm(g[n]) > 0 for n in rep.unary.shapes) == len(rep.unary.shapes)
    np.testing.assert_array_equal(rep.pair_var('kernel').cpu().numpy(), params[OD.PAIR_PREFIX + 'kernel'])


def test_everything_after_z_is_the_patch_replicas():
    """train_pairwise, pairwise_texture and holes together: given the same z, the loss, dz and the pairwise gradients of
    the two forms are the same bits; then the step of the fcsp form runs."""
    from ann3depth_amd import models, ops
    img, dep = random_batch(1, 22)
    dep[:, :12] = 1.0                                                   # above the range cap: a band of holes
    img, dep = torch.from_numpy(img).cuda(), torch.from_numpy(dep).cuda()
    kw = dict(train_pairwise=True, pairwise_texture=True, valid_range=(0.0, 0.99), seed=9)
    a = models.DCNFReplica(1, unary='fcsp', **kw)
    b = models.DCNFReplica(1, **kw)
    assert same_bits(a.pair_group.var, b.pair_group.var)
    a.forward(img, dep)
    b.unary.forward(img)
    b.unary.z.copy_(a.unary.z)
    b.forward_crf(dep)
    for rep in (a, b):
        ops.pair_dense_bwd(rep.sims, rep.dr, rep.pair_grad('kernel'), rep.pair_grad('bias'))
    torch.cuda.synchronize()
    assert 0 < int(a.nobs[0]) < 48 and torch.equal(a.nobs, b.nobs)
    for x, y in ((a.loss, b.loss), (a.dz, b.dz), (a.dr, b.dr), (a.sims, b.sims), (a.r, b.r), (a.pair_group.grad, b.pair_group.grad)):
        assert same_bits(x, y)
    assert float(a.pair_group.grad.abs().max()) > 0
    grads, before = a.pair_group.grad.clone(), a.unary.group.var.clone()
    out = a.step(img, dep)
    torch.cuda.synchronize()
    assert np.isfinite(float(out['mean_loss'])) and same_bits(a.pair_group.grad, grads)
    assert torch.isfinite(a.unary.group.grad).all() and float(a.unary.group.grad.abs().max()) > 0
    assert not torch.equal(a.unary.group.var, before) and a.global_step == 1


def test_the_default_is_the_patch_form_bit_for_bit():
    from ann3depth_amd import models
    img, dep = (torch.from_numpy(v).cuda() for v in random_batch(1, 23))
    a, b = models.DCNFReplica(1, seed=4), models.DCNFReplica(1, seed=4, unary='patch')
    assert type(a.unary) is models.DCNFUnary and type(b.unary) is models.DCNFUnary and a.unary_form == b.unary_form == 'patch'
    la, lb = a.step(img, dep)['mean_loss'], b.step(img, dep)['mean_loss']
    torch.cuda.synchronize()
    assert same_bits(la, lb) and same_bits(a.unary.group.var, b.unary.group.var) and same_bits(a.unary.group.grad, b.unary.group.grad)
    assert a.unary.var('dense/kernel').shape == (12544, 128)


def _write_records(path, count, seed):
    from ann3depth_amd import tfrecord
    rng = np.random.default_rng(seed)
    with tfrecord.TFRecordWriter(path) as w:
        for _ in range(count):
            w.write_example(rng.random((48, 64, 3)).astype(np.float32), rng.random((6, 8, 1)).astype(np.float32))


def test_driver_checkpoint_and_evaluate(tmp_path, capsys):
    from ann3depth_amd import ann3depth, evaluate, models
    root = str(tmp_path / 'data')
    os.makedirs(os.path.join(root, 'nyu'))
    _write_records(os.path.join(root, 'nyu', 'train.tfrecords'), 8, 1)
    _write_records(os.path.join(root, 'nyu', 'test.tfrecords'), 4, 2)
    ck = str(tmp_path / 'ckpt')
    common = ['nyu', '--steps', '3', '--batchsize', '2', '--datadir', root, '--ckptdir', ck, '--sumfreq', '1', '--ckptfreq', '0']
    try:
        assert ann3depth.main(common + ['--model', 'msdn', '--unary', 'fcsp']) == 2          # refused: msdn has no unary part
        assert not os.path.exists(os.path.join(ck, 'msdn'))
        assert ann3depth.main(common + ['--model', 'dcnf', '--unary', 'fcsp']) == 0
        assert models.dcnf.unary == 'fcsp'
        assert ann3depth.main(common + ['--model', 'dcnf', '--id', 'patch', '--steps', '1']) == 0
        assert models.dcnf.unary == 'patch'
        # resuming across the flag is refused, both ways
        with pytest.raises(ValueError, match=r'has shape \[256, 128\], this replica.s is \[12544, 128\].*--unary fcsp'):
            ann3depth.main(common + ['--model', 'dcnf', '--steps', '4'])
        with pytest.raises(ValueError, match=r'has shape \[12544, 128\], this replica.s is \[256, 128\]'):
            ann3depth.main(common + ['--model', 'dcnf', '--id', 'patch', '--steps', '2', '--unary', 'fcsp'])
    finally:
        models.dcnf.unary = 'patch'
    capsys.readouterr()
    d = os.path.join(ck, 'dcnf')
    recs = [json.loads(l) for l in open(os.path.join(d, 'summaries.jsonl'))]
    assert [r['global_step'] for r in recs] == [1, 2, 3] and all(np.isfinite(r['loss/mean_loss']) for r in recs)
    sd = torch.load(os.path.join(d, 'model.ckpt-3.pt'))
    assert tuple(sd[DENSE].shape) == (256, 128)
    base = ['--model', 'dcnf', '--batchsize', '2', '--ckptdir', ck, '--datadir', root]
    assert evaluate.main(base + ['nyu']) == 0
    got = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert got['unary_form'] == 'fcsp' and got['records'] == 4 and got['global_step'] == 3
    assert np.isfinite(got['crf_nll']) and got['singular_systems'] == 0
    for o in ('unary', 'crf'):
        assert got[o] and all(np.isfinite(v) for v in got[o].values())
    assert evaluate.main(base + ['--id', 'patch', 'nyu']) == 0
    two = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert 'unary_form' not in two and two['records'] == 4 and two['global_step'] == 1


def test_restore_across_the_forms_and_the_warm_start():
    from ann3depth_amd import models
    fcsp, patch = models.DCNFReplica(1, unary='fcsp', seed=2), models.DCNFReplica(1, seed=3)
    for src, dst, pattern in ((patch, fcsp, r'has shape \[12544, 128\], this replica.s is \[256, 128\]'),
                              (fcsp, patch, r'has shape \[256, 128\], this replica.s is \[12544, 128\]')):
        before = dst.unary.group.var.clone()
        with pytest.raises(ValueError, match=pattern):
            dst.load_state_dict(src.state_dict())
        with pytest.raises(ValueError, match=pattern):
            dst.load_tf_variables(src.tf_variables())
        with pytest.raises(ValueError, match=pattern):
            models.DCNFReplica(1, params=src.tf_variables(), unary=dst.unary_form)
        assert same_bits(dst.unary.group.var, before) and dst.global_step == 0            # nothing was copied
    fcsp.load_state_dict(models.DCNFReplica(1, unary='fcsp', seed=4).state_dict())        # its own form loads
    before = {n: fcsp.unary.group.view(fcsp.unary.group.var, n).clone() for n in fcsp.unary.shapes}
    names = fcsp.unary.load_convs_from(patch.state_dict())
    assert sorted(names) == sorted(n for n in fcsp.unary.shapes if '/conv2d' in n) and len(names) == 10
    for n in fcsp.unary.shapes:
        now = fcsp.unary.group.view(fcsp.unary.group.var, n)
        if n in names:
            assert same_bits(now, patch.unary.group.view(patch.unary.group.var, n))
        else:
            assert same_bits(now, before[n])
    assert not same_bits(fcsp.unary.var('conv2d/kernel'), before[OD.PREFIX + 'conv2d/kernel'])


def test_two_ranks_stay_identical_and_match_the_one_rank_step(tmp_path):
    """tests/fcsp_dp_worker.py: two ranks on the one GPU over gloo (as the other two-rank DCNF tests run, so nothing is
    skipped on a single card), one image each, two steps; the one-rank replica takes both images."""
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / 'ok.txt')
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), A3D_DIST_BACKEND='gloo')
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, 'fcsp_dp_worker.py'), out], env=env))
    for p in procs:
        assert p.wait(timeout=300) == 0
    assert open(out).read() == '1'
